"""Operands off the allocator's alignment, for tests/test_operand_placement_gpu.py.

`_chk` in rba_amd.ops demands contiguity, not alignment: `big[1:1 + n]` is a legal argument 4 bytes off a 16-byte boundary.  `shifted(t, nbytes)` builds such
an argument with known surroundings: a contiguous tensor equal to `t`, carved out of a byte buffer filled with 0xFF (NaN for floats, 255 for uint8, -1 for
integers -- the poison of tests/_guard.py), whose data_ptr() is `nbytes` past a 16-byte boundary.  A kernel that rounds the pointer down, or reads beside the
tensor into a result, meets NaN; one that writes beside it changes a guard byte, which `untouched()` finds."""
import torch

HEAD = 4096            # guard bytes in front of the payload (the shift is taken out of the first 16 of the payload's own 16-byte line)
TAIL = 4096
POISON = 0xFF
SHIFTS = {torch.float32: (4, 8, 12), torch.int32: (4, 8, 12), torch.int64: (8,), torch.uint8: (1, 2, 3, 5), torch.float16: (4, 8, 12), torch.bfloat16: (4, 8, 12)}


class Placed:
    """a shifted tensor with the buffer it was carved out of"""

    def __init__(self, raw, start, nbytes, tensor):
        self.raw, self.start, self.nbytes, self.tensor = raw, start, nbytes, tensor

    def untouched(self):
        """True when every byte beside the payload is still the poison"""
        torch.cuda.synchronize()
        head, tail = self.raw[:self.start], self.raw[self.start + self.nbytes:]
        return bool((head == POISON).all().item()) and bool((tail == POISON).all().item())


def place(t, nbytes):
    """-> Placed: `t`'s values, contiguous, at data_ptr() % 16 == nbytes % 16, between HEAD and TAIL guard bytes"""
    assert t.is_cuda and nbytes % t.element_size() == 0, "a shift moves whole elements"
    n = t.numel() * t.element_size()
    raw = torch.empty(HEAD + 16 + n + 16 + TAIL, dtype=torch.uint8, device=t.device)
    raw.fill_(POISON)
    assert raw.data_ptr() % 16 == 0
    start = HEAD + nbytes
    out = raw[start:start + n].view(t.dtype).view(t.shape)
    out.copy_(t)
    assert out.is_contiguous() and out.data_ptr() % 16 == nbytes % 16 and torch.equal(out, t)
    return Placed(raw, start, n, out)


def shifted(t, nbytes):
    """the tensor alone (its buffer stays alive through it)"""
    return place(t, nbytes).tensor


# ---- the K1 cases of the placement test, (Q, K, H, W, seed), and what an argmax comparison may leave out: kept here so that the seeds are checked without a device
K1_CASES = {"rba_reduce[K=3]": (5, 3, 8, 8, 5003), "rba_reduce[K=19]": (7, 19, 8, 8, 7019)}
K1_SEM_SEG_BAR = 5e-6           # test_kernels_gpu.py::test_k1_shapes
ARGMAX_LEFT_OUT_CAP = 0.01


def k1_inputs(name):
    """(mask_pred [Q,H,W], cls_prob [Q,K]) fp32 on the CPU"""
    import torch.nn.functional as F
    Q, K, H, W, seed = K1_CASES[name]
    g = torch.Generator().manual_seed(seed)
    mp = torch.randn(Q, H, W, generator=g) * 5
    return mp, F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()


def decided_pixels(sem64, bar):
    """(pixels whose fp64 top-two gap exceeds `bar`, the share left out)"""
    top2 = sem64.topk(2, dim=0).values
    decided = (top2[0] - top2[1]) > bar
    return decided, 1.0 - decided.double().mean().item()


UP4_CASE = (7, 19, 2, 4)        # (Q, K, h, w) of the rba_reduce_up4 case: K = 19 and a crop width of 16, the matrix-pipe form
UP4_SEM_SEG_BAR = 1e-5          # test_kernels_gpu.py::test_k1_up4_shapes


def up4_inputs():
    """(mask_lowres [Q,h,w], cls_prob [Q,K]) fp32 on the CPU"""
    import torch.nn.functional as F
    Q, K, h, w = UP4_CASE
    g = torch.Generator().manual_seed(h * 100 + w)
    low = torch.randn(Q, h, w, generator=g) * 5
    return low, F.softmax(torch.randn(Q, K + 1, generator=g) * 3, -1)[:, :-1].contiguous()
