"""K12b on the GPU: ops.resize_u8_pil_bilinear against the numpy restatement of Pillow's Image.resize(BILINEAR) (tests/_tta_cases.py, held against Pillow
itself in test_tta_cpu.py) -- equal in every byte, with and without the folded horizontal flip."""
import numpy as np
import pytest
import torch

from tests import _tta_cases as G

pytestmark = pytest.mark.gpu
_id = lambda s: "{}x{}to{}x{}".format(*s[0], *s[1])


def _poison():
    for n in (1 << 10, 1 << 16, 1 << 20):
        torch.full((n,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()


@pytest.mark.parametrize("flip", [False, True], ids=["plain", "flip"])
@pytest.mark.parametrize("i", range(len(G.RESIZE_SHAPES)), ids=[_id(s) for s in G.RESIZE_SHAPES])
def test_every_byte_equals_the_restatement(i, flip):
    from rba_amd import ops
    (h, w), (H, W) = G.RESIZE_SHAPES[i]
    img, want = G.resize_case(i)
    x = torch.from_numpy(img).cuda()
    _poison()
    out = ops.resize_u8_pil_bilinear(x, (H, W), flip=flip)
    assert out.dtype == torch.uint8 and tuple(out.shape) == (3, H, W) and out.is_contiguous()
    got = out.cpu().numpy()
    assert np.array_equal(got, want[:, :, ::-1] if flip else want), int((got != (want[:, :, ::-1] if flip else want)).sum())
    assert torch.equal(x.cpu(), torch.from_numpy(img))                                     # the input is left as it was
    _poison()
    assert torch.equal(ops.resize_u8_pil_bilinear(x, (H, W), flip=flip), out)              # two runs, equal bytes


@pytest.mark.parametrize("i", range(len(G.RESIZE_SHAPES)), ids=[_id(s) for s in G.RESIZE_SHAPES])
def test_the_flipped_output_is_the_flip_of_the_unflipped_one(i):
    from rba_amd import ops
    (h, w), (H, W) = G.RESIZE_SHAPES[i]
    x = torch.from_numpy(G.resize_case(i)[0]).cuda()
    assert torch.equal(ops.resize_u8_pil_bilinear(x, (H, W), flip=True), ops.resize_u8_pil_bilinear(x, (H, W)).flip(-1))


def test_word_stores_and_several_workgroups_per_row():
    """a row of more than 256 four-column groups, its width a multiple of four (the 32-bit stores) and not; one and four channels"""
    from rba_amd import ops
    rng = np.random.default_rng(11)
    for C, (h, w), (H, W) in ((1, (3, 700), (5, 1040)), (4, (4, 1300), (2, 1027)), (3, (6, 1040), (6, 2080))):
        img = rng.integers(0, 256, (C, h, w), dtype=np.uint8)
        want = G.pil_bilinear_resize(img, (H, W))
        x = torch.from_numpy(img).cuda()
        for flip in (False, True):
            _poison()
            got = ops.resize_u8_pil_bilinear(x, (H, W), flip=flip).cpu().numpy()
            assert np.array_equal(got, want[:, :, ::-1] if flip else want), (C, h, w, H, W, flip)


def test_refusals():
    from rba_amd import ops
    from rba_amd._lib import RbaHipError
    x = torch.zeros(3, 4, 5, dtype=torch.uint8, device="cuda")
    for bad in (x.cpu(), x.float(), x[0], x[:, :, ::2], torch.zeros(3, 0, 5, dtype=torch.uint8, device="cuda")):
        with pytest.raises(RbaHipError):
            ops.resize_u8_pil_bilinear(bad, (6, 7))
    for size in ((0, 7), (6, 0)):
        with pytest.raises(RbaHipError):
            ops.resize_u8_pil_bilinear(x, size)
