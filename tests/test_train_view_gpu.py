"""K14 (ops.train_view, csrc/train_view.hip) on the GPU: every output byte or element equal to the composition of tests/_train_view_cases.py -- the
resize cases (both passes, one, none; staged and unstaged; byte and word stores; several workgroups per row and per column), the crop offsets, the
flip, the paste, every colour leg at its extremes and the lattice of all {0,5,..,255}^3 triples, the canvas, the label table, the histogram, bitwise
reproducibility, and the refusals.  No tolerance anywhere."""
import pytest
import torch

from tests import _train_view_cases as C

pytestmark = pytest.mark.gpu


def _run(img, lab, p, obj=None, objmask=None, lut=None, pad_size=None):
    from rba_amd import ops
    dev = [None if t is None else t.cuda() for t in (img, lab, obj, objmask, lut)]
    return ops.train_view(dev[0], dev[1], p, dev[2], dev[3], dev[4], C.IGNORE, C.OOD, pad_size)


@pytest.mark.parametrize("name", sorted(C.GEOMETRY))
def test_geometry_with_and_without_flip(name):
    img, lab = C.frame(*C.GEOMETRY[name][0])
    plain, flipped = C.params_of(name), C.params_of(name, flip=True)
    want = C.ref_view(img, lab, plain)
    got, got_f = _run(img, lab, plain), _run(img, lab, flipped)
    C.check_equal(got, want, name)
    C.check_equal(got_f, C.ref_view(img, lab, flipped), name + " flipped")
    for a, b in zip(got[:3], got_f[:3]):
        assert torch.equal(a.flip(-1), b)
    assert torch.equal(got[3], got_f[3])
    ch, cw = C.GEOMETRY[name][2][2:]
    assert torch.equal(got[3].cpu().long(), torch.bincount(want[1][:ch, :cw].reshape(-1), minlength=256))


@pytest.mark.parametrize("flip", (False, True))
@pytest.mark.parametrize("paste", sorted(C.PASTES))
def test_paste(paste, flip):
    (bh, bw), holes, pos, geometry = C.PASTES[paste]
    img, lab = C.frame(24, 48)
    obj, objmask = C.ood_object(bh, bw, holes)
    p = C.params_of(geometry, flip=flip, paste=pos)
    want = C.ref_view(img, lab, p, obj, objmask)
    assert 0 < int(want[3][C.OOD]) and (paste == "covers_crop" or int(want[3][C.OOD]) < 12 * 24)
    C.check_equal(_run(img, lab, p, obj, objmask), want, paste)
    # the same decisions without an object (ood_index drawn, bh = 0: no paste) give the unpasted view
    none = C.params_of(geometry, flip=flip)
    C.check_equal(_run(img, lab, none, obj, objmask), C.ref_view(img, lab, none), paste + " absent")


def test_paste_through_every_resize():
    img, lab = C.frame(24, 48)
    obj, objmask = C.ood_object(9, 13, True)
    for name in ("e12_whole", "e17_whole", "e24_inside", "e48_inside", "x_only_down", "y_only_up"):
        p = C.params_of(name, flip=name.endswith("whole"), paste=(6, 12))
        C.check_equal(_run(img, lab, p, obj, objmask), C.ref_view(img, lab, p, obj, objmask), name)
    img, lab = C.frame(80, 48)                                       # the unstaged form
    p = C.params_of("tall_to_10", paste=(30, 10))
    C.check_equal(_run(img, lab, p, obj, objmask), C.ref_view(img, lab, p, obj, objmask), "tall_to_10")


@pytest.mark.parametrize("name", sorted(C.color_cases()))
def test_colour_legs(name):
    c = C.color_cases()[name]
    img, lab = C.frame(24, 48)
    for geometry in ("e31_inside", "e24_first"):
        p = C.params_of(geometry, flip=geometry == "e24_first", color=c)
        C.check_equal(_run(img, lab, p), C.ref_view(img, lab, p), f"{name} {geometry}")
    img, lab = C.primaries()
    from rba_amd.dataset_mappers import TrainViewParams
    p = TrainViewParams(new_h=2, new_w=4, crop=(0, 0, 2, 4), color=c)
    C.check_equal(_run(img, lab, p), C.ref_view(img, lab, p), f"{name} primaries")


@pytest.mark.parametrize("name", ("all_order0", "all_order1", "saturation_1.5", "saturation_0.5", "hue_18", "hue_-18", "hue_0", "brightness_-32.0",
                                  "contrast_1.5"))
def test_colour_legs_on_the_lattice(name):
    """every {0,5,..,255}^3 triple, no resize"""
    from rba_amd.dataset_mappers import TrainViewParams
    img, lab = C.lattice()
    p = TrainViewParams(new_h=376, new_w=374, crop=(0, 0, 376, 374), color=C.color_cases()[name])
    C.check_equal(_run(img, lab, p), _lattice_truth(name), name)


_LATTICE = {}


def _lattice_truth(name):
    from rba_amd.dataset_mappers import TrainViewParams
    if name not in _LATTICE:
        img, lab = C.lattice()
        _LATTICE[name] = C.ref_view(img, lab, TrainViewParams(new_h=376, new_w=374, crop=(0, 0, 376, 374), color=C.color_cases()[name]))
    return _LATTICE[name]


def test_canvas_and_label_table():
    from rba_amd.sem_seg_datasets import cityscapes_lut
    img, lab = C.frame(24, 48, raw_ids=True)
    obj, objmask = C.ood_object(6, 9)
    lut = cityscapes_lut()
    for name, pad in (("e31_inside", (32, 32)), ("odd_inside", None), ("e17_whole", (32, 35)), ("e24_last", (13, 24))):
        src = C.GEOMETRY[name][0]
        img, lab = C.frame(*src, raw_ids=True)
        p = C.params_of(name, flip=True, color=C.color_cases()["all_order1"], paste=(7, 14))
        got, want = _run(img, lab, p, obj, objmask, lut, pad), C.ref_view(img, lab, p, obj, objmask, lut, pad_size=pad)
        C.check_equal(got, want, name)
        ch, cw = C.GEOMETRY[name][2][2:]
        assert tuple(got[2].shape) == (ch, cw) and tuple(got[0].shape[1:]) == (pad or (ch, cw))
        if pad == (32, 32):
            assert bool((got[0][:, ch:] == 128).all()) and bool((got[0][:, :, cw:] == 128).all())
            assert bool((got[1][ch:] == C.IGNORE).all()) and bool((got[1][:, cw:] == C.IGNORE).all())
            assert set(got[1][:ch, :cw].unique().tolist()) <= set(range(19)) | {C.IGNORE, C.OOD}


def test_other_ignore_and_ood_labels():
    from rba_amd import ops
    img, lab = C.frame(24, 48)
    obj, objmask = C.ood_object(6, 9)
    objmask = torch.where(objmask == C.OOD, torch.tensor(77, dtype=torch.uint8), objmask)
    p = C.params_of("e31_inside", paste=(7, 14))
    plain = C.ref_view(img, lab, p, obj, objmask, None, C.IGNORE, 77)[1]
    ign = int(plain[plain < 19].mode().values)                   # a class the crop does show stands in for the ignored label
    got = ops.train_view(img.cuda(), lab.cuda(), p, obj.cuda(), objmask.cuda(), None, ign, 77, (16, 28))
    C.check_equal(got, C.ref_view(img, lab, p, obj, objmask, None, ign, 77, (16, 28)), f"labels {ign} / 77")
    assert int((got[2] == 1).sum()) > 0 and int((got[2] == ign).sum()) > 0 and int((got[1][12:] == ign).sum()) == 4 * 28


def test_two_runs_give_equal_bits_and_stale_outputs_do_not_matter():
    img, lab = C.frame(40, 48)
    obj, objmask = C.ood_object(9, 13, True)
    p = C.params_of("two_row_tiles", flip=True, color=C.color_cases()["all_order0"], paste=(11, 20))
    a = _run(img, lab, p, obj, objmask)
    junk = [torch.full((4096,), 0x7f7f7f7f, dtype=torch.int32, device="cuda") for _ in range(8)]      # leave other bits in the freed blocks
    del junk
    b = _run(img, lab, p, obj, objmask)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    C.check_equal(a, C.ref_view(img, lab, p, obj, objmask), "two_row_tiles")


def test_refusals():
    from rba_amd import ops
    from rba_amd.dataset_mappers import TrainViewParams
    img, lab = (t.cuda() for t in C.frame(24, 48))
    obj, objmask = (t.cuda() for t in C.ood_object(6, 9))
    ok = C.params_of("e31_inside")
    ops.train_view(img, lab, ok)
    for crop in ((20, 0, 12, 24), (0, 39, 12, 24), (-1, 0, 12, 24), (0, 0, 32, 24)):                  # a crop outside the resized frame
        with pytest.raises(ops.RbaHipError):
            ops.train_view(img, lab, TrainViewParams(new_h=31, new_w=62, crop=crop))
    for pos in ((19, 0), (0, 40), (-1, 0)):                                                           # a box outside the source
        with pytest.raises(ops.RbaHipError):
            ops.train_view(img, lab, C.params_of("e31_inside", paste=pos), obj, objmask)
    with pytest.raises(ops.RbaHipError, match="canvas"):
        ops.train_view(img, lab, ok, pad_size=(11, 24))
    with pytest.raises(ops.RbaHipError, match="HIP"):
        ops.train_view(img.cpu(), lab, ok)
    with pytest.raises(ops.RbaHipError, match="HIP"):
        ops.train_view(img, lab.cpu(), ok)
    with pytest.raises(ops.RbaHipError, match="contiguous"):
        ops.train_view(img.flip(0).permute(0, 2, 1)[:, :24, :24].permute(0, 2, 1), lab[:, :24].contiguous(), ok)
    with pytest.raises(ops.RbaHipError, match="contiguous"):
        ops.train_view(img, lab.t().contiguous().t(), ok)
    with pytest.raises(ops.RbaHipError, match="uint8"):
        ops.train_view(img.float(), lab, ok)
    with pytest.raises(ops.RbaHipError, match="uint8"):
        ops.train_view(img, lab.long(), ok)
    with pytest.raises(ops.RbaHipError, match="lab"):
        ops.train_view(img, lab[:23].contiguous(), ok)
    with pytest.raises(ops.RbaHipError, match="objmask"):
        ops.train_view(img, lab, C.params_of("e31_inside", paste=(0, 0)), obj, objmask[:5].contiguous())
    with pytest.raises(ops.RbaHipError, match="obj"):
        ops.train_view(img, lab, C.params_of("e31_inside", paste=(0, 0)))
    with pytest.raises(ops.RbaHipError, match="256"):
        ops.train_view(img, lab, ok, lut=torch.zeros(255, dtype=torch.uint8, device="cuda"))
