"""The window machinery of the GPU conformance matrices (tests/test_gpu_sage_rows_matrix.py,
tests/test_gpu_spmm_matrix.py, tests/test_gpu_dense_matrix.py, tests/test_gpu_gemm_b16_matrix.py, tests/test_gpu_pool_matrix.py): outputs as NaN-filled windows inside guarded allocations
(integer outputs: sentinel-filled windows, IntWin), inputs with NaN after their last row, the comparison against an fp64 reference under a per-element bound
with the largest err / bound kept per section, and the amax check."""
import torch

from sage_rows_ref import D, ratio

PATTERN = 0x4B1D5EED    # guard bit pattern (as f32: 1.03e7, finite)
NAN = float("nan")
RATIOS = {}             # section -> largest err / bound seen


def ceil4(x):
    return (x + 3) // 4 * 4


class Out:
    """A rows x cols f32 output window (row stride ld) inside a guarded allocation: two guard rows
    above and below and the ld padding hold PATTERN; the window starts as NaN or as `init`."""

    def __init__(self, dev, rows, cols, ld=None, init=None):
        self.rows, self.cols = rows, cols
        self.ld = ld = ceil4(cols) + 4 if ld is None else ld
        off = 2 * ld
        self.idx = (off + torch.arange(rows).view(rows, 1) * ld + torch.arange(cols).view(1, cols)).to(dev)
        self.buf = torch.empty((rows + 4) * ld, dtype=torch.float32, device=dev)
        self.buf.view(torch.int32).fill_(PATTERN)
        self.buf[self.idx] = NAN if init is None else init.to(dev).view(rows, cols)
        self.ptr = self.buf.data_ptr() + 4 * off

    def read(self):
        return self.buf[self.idx].cpu()

    def guard(self, label):
        g = self.buf.view(torch.int32).clone()
        g[self.idx] = PATTERN
        bad = (g != PATTERN).nonzero().flatten()
        assert bad.numel() == 0, (f"{label}: {bad.numel()} guard elements outside the {self.rows} x {self.cols} "
                                  f"window (ld {self.ld}) overwritten; first at flat offset {int(bad[0])}")


class OutB16:
    """n bf16 output elements starting as NaN (0x7FC0), 64 guard elements of PATTERN16 on either side (the
    window starts on a 16-byte boundary)"""
    PATTERN16 = 0x4B1D    # (as bf16: 1.03e7, finite)
    GUARD = 64

    def __init__(self, dev, n):
        self.n = n
        self.buf = torch.full((n + 2 * self.GUARD,), self.PATTERN16, dtype=torch.int16, device=dev)
        self.buf[self.GUARD:self.GUARD + n] = 0x7FC0
        self.ptr = self.buf.data_ptr() + 2 * self.GUARD

    def read(self):
        return self.buf[self.GUARD:self.GUARD + self.n].cpu().view(torch.bfloat16)

    def guard(self, label):
        g = torch.cat([self.buf[:self.GUARD], self.buf[self.GUARD + self.n:]])
        bad = (g != self.PATTERN16).nonzero().flatten()
        assert bad.numel() == 0, f"{label}: {bad.numel()} bf16 guard elements around the {self.n}-element window overwritten"


def inp16(dev, t, pad=2):
    """a bf16 [rows, cols] input on the device with NaN in `pad` rows after its last"""
    buf = torch.full((t.size(0) + pad, t.size(1)), NAN, dtype=torch.bfloat16)
    buf[:t.size(0)] = t
    return buf.to(dev)


def scalar(dev, v):
    return Out(dev, 1, 1, init=torch.tensor([float(v)]))


def inp(dev, t, pad=2):
    """an input on the device with NaN after its last row (float) -- a read past n_rows poisons"""
    if t is None:
        return None
    if not t.is_floating_point():
        return t.to(dev)
    t2 = t.view(t.size(0), -1)
    buf = torch.full((t2.size(0) + pad, t2.size(1)) if t.dim() > 1 else (t.numel() + 8,), NAN)
    buf.view(-1)[:t.numel()] = t.reshape(-1)
    return buf.to(dev)


class In:
    """An f32 [rows, cols] input with row stride ld >= cols: NaN in the ld padding, in two rows after
    the last one and in `lead` floats before the first (lead = 1: a base pointer 4 bytes past a 16-byte
    boundary) -- a read outside the rows' columns poisons."""

    def __init__(self, dev, t, ld=None, lead=0):
        rows, cols = t.shape
        self.ld = ld = ceil4(cols) + 4 if ld is None else ld
        host = torch.full((4 + lead + (rows + 2) * ld,), NAN)
        host[4 + lead:4 + lead + rows * ld].view(rows, ld)[:, :cols] = t
        self.buf = host.to(dev)
        self.ptr = self.buf.data_ptr() + 4 * (4 + lead)


class Win:
    """A rows x cols output window of f32 or bf16 elements (row stride ld, its first element `shift` elements
    past a 16-byte boundary) inside an allocation that holds the 32-bit PATTERN: at least two guard rows
    above and below and the ld padding; the window starts as NaN or as `init`. The guard is compared in
    the element's own width (a bf16 window: as 16-bit words, 0x5EED / 0x4B1D alternating)."""

    def __init__(self, dev, rows, cols, ld, dtype=torch.float32, shift=0, init=None):
        self.rows, self.cols, self.ld, self.dtype = rows, cols, ld, dtype
        bf = dtype == torch.bfloat16
        self.ity = torch.int16 if bf else torch.int32
        off = (2 * ld + 7) // 8 * 8 + 8 + shift
        n = (off + (rows + 2) * ld + 16 + 1) // 2 * 2
        words = torch.full((n // 2 if bf else n,), PATTERN, dtype=torch.int32, device=dev)
        self.raw = words.view(self.ity)
        self.expect = self.raw.clone()
        self.idx = (off + torch.arange(rows).view(rows, 1) * ld + torch.arange(cols).view(1, cols)).to(dev)
        if init is None:
            self.raw[self.idx] = 0x7FC0 if bf else 0x7FC00000
        else:
            self.raw[self.idx] = init.to(dtype).contiguous().view(self.ity).view(rows, cols).to(dev)
        self.ptr = words.data_ptr() + (2 if bf else 4) * off

    def read(self):
        return self.raw[self.idx].cpu().view(self.dtype)

    def guard(self, label):
        g = self.raw.clone()
        g[self.idx] = self.expect[self.idx]
        bad = (g != self.expect).nonzero().flatten()
        assert bad.numel() == 0, (f"{label}: {bad.numel()} guard elements outside the {self.rows} x {self.cols} "
                                  f"{self.dtype} window (ld {self.ld}) overwritten; first at flat offset {int(bad[0])}, "
                                  f"window at {int(self.idx[0, 0]) if self.idx.numel() else 0}")


class IntWin:
    """A window of n int32 / int64 / uint8 elements pre-filled with a sentinel no valid result can equal
    (-0x5EED; 0xA5 for uint8), inside an allocation whose `pad` guard elements on either side hold a second
    pattern (PATTERN, PATTERN twice, 0x5A). pad is a multiple of 64 elements, so the window starts as
    aligned as the allocation (a workspace: at least 64 bytes)."""
    SENTINEL = {torch.int32: -0x5EED, torch.int64: -0x5EED, torch.uint8: 0xA5}
    GUARD = {torch.int32: PATTERN, torch.int64: PATTERN << 32 | PATTERN, torch.uint8: 0x5A}

    def __init__(self, dev, n, dtype=torch.int32, pad=64):
        assert pad % 64 == 0 and pad > 0
        self.n, self.pad, self.dtype = n, pad, dtype
        self.sentinel, self.pattern = self.SENTINEL[dtype], self.GUARD[dtype]
        self.buf = torch.full((n + 2 * pad,), self.pattern, dtype=dtype, device=dev)
        self.buf[pad:pad + n] = self.sentinel
        self.ptr = self.buf.data_ptr() + pad * self.buf.element_size()

    def read(self):
        return self.buf[self.pad:self.pad + self.n].cpu()

    def guard(self, label):
        g = torch.cat([self.buf[:self.pad], self.buf[self.pad + self.n:]])
        bad = (g != self.pattern).nonzero().flatten()
        assert bad.numel() == 0, (f"{label}: {bad.numel()} guard elements around the {self.n}-element {self.dtype} "
                                  f"window overwritten; first at {int(bad[0]) - self.pad if int(bad[0]) < self.pad else int(bad[0]) - self.pad + self.n} "
                                  f"relative to the window's start")

    def assert_all_written(self, label, upto=None):
        """no sentinel is left in the first `upto` (default: all n) elements"""
        upto = self.n if upto is None else upto
        left = (self.read()[:upto] == self.sentinel).nonzero().flatten()
        assert left.numel() == 0, f"{label}: {left.numel()} of the first {upto} elements never written; first at {int(left[0])}"

    def assert_untouched(self, label, start=0):
        """the elements from `start` on still hold the sentinel"""
        hit = (self.read()[start:] != self.sentinel).nonzero().flatten()
        assert hit.numel() == 0, (f"{label}: {hit.numel()} elements behind the first {start} of the {self.n}-element window "
                                  f"written; first at {start + int(hit[0])}")


class Buf:
    """An f32 or bf16 [rows, cols] input with row stride ld >= cols, its first element `shift` elements past
    a 16-byte boundary: NaN in the ld padding, before the first row and in two rows after the last -- a
    read outside the rows' columns poisons."""

    def __init__(self, dev, t, ld=None, dtype=torch.float32, shift=0):
        rows, cols = t.shape
        self.ld = ld = cols if ld is None else ld
        assert ld >= cols
        host = torch.full((8 + shift + (rows + 2) * ld + 8,), NAN, dtype=dtype)
        host[8 + shift:8 + shift + rows * ld].view(rows, ld)[:, :cols] = t.to(dtype)
        self.buf = host.to(dev)
        self.ptr = self.buf.data_ptr() + host.element_size() * (8 + shift)


def ptr(t):
    return None if t is None else (t.ptr if hasattr(t, "ptr") else t.data_ptr())


def check(sec, out, ref, bound, label):
    fin = torch.isfinite(out)
    assert bool(fin.all()), f"{label}: {int((~fin).sum())} elements not finite (never written, or a read past an " \
                            f"input's end); first at {(~fin).nonzero()[0].tolist()}"
    err = (out.to(D) - ref).abs()
    r = ratio(err, bound)
    RATIOS[sec] = max(RATIOS.get(sec, 0.0), r)
    over = err - bound
    if bool((over > 0).any()):
        i = (over.view(-1).argmax()).item()
        raise AssertionError(f"{label}: {int((over > 0).sum())} elements over the bound (err / bound {r:.3f}); worst "
                             f"at flat {i}: got {out.view(-1)[i].item():.9g}, fp64 {ref.reshape(-1)[i].item():.9g}, "
                             f"|err| {err.view(-1)[i].item():.3g} > {bound.reshape(-1)[i].item():.3g}")


def amax_prev(i):
    """alternate: a previous value of 0, and one above every maximum"""
    return 0.0 if i % 2 == 0 else 3.0e30


def check_amax(am, prev, out, label):
    am.guard(label + " amax")
    want = max(torch.tensor(prev, dtype=torch.float32).item(), out.abs().max().item() if out.numel() else 0.0)
    assert am.read().item() == want, f"{label}: amax {am.read().item()!r} != max(previous {prev}, max |output|) = {want!r}"
