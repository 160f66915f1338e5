"""GPU: the epilogue's two C store shapes (BGNN_TUNE_GEMM_CSTORE: 0 = 32-column blocks, 128-B row
pieces; 1 = 16-row blocks, whole row segments of the wave tile) on the same operands.

Every case runs under both knob values and checks
  * bit identity, old shape against new (torch.equal on C, equal c_amax where it is folded),
  * the window: C has ldc = N + 12 inside a buffer filled with a guard pattern; rows at and beyond
    M, the 12 pad columns and the elements before and after keep the pattern under both shapes,
  * fp64: |c - ref| <= REL * mag + TINY per element, tests/test_gpu_gemm_matrix.py's class and
    magnitude (|alpha| |A||B| + |beta| |C0| + |bias| + |drop(src)| + |gathered rows|).
Cases: the forward family on the pre-split weight path (256 x 256 tile: two interior row tiles
and a ragged one), the pipelined kernel plain (knob 16 = 2 and 3), the drop-add epilogue at
p = 0 and 0.1 on the LDS-source path and on the prefetched-source path, alpha / beta (C as the
addend) / bias / ReLU, gathered rows, and the tall 128 x 128 tile (32-column wave tiles)."""
import pytest
import torch

from bgnn import _lib
from bgnn.graph import _stream

pytestmark = pytest.mark.gpu

TINY = 1e-37
REL = 2e-6              # tests/test_gpu_gemm_matrix.py's per-element class
PATTERN = 0x4B1D5EED    # guard bit pattern (finite as f32)
PAD = 12                # ldc = N + PAD
GUARD_ROWS = 3          # whole guard rows above the window and below row M - 1
KNOB_CSTORE = 17
KNOB_BDMA = 16
SEED = 1234


@pytest.fixture(autouse=True)
def _restore_knobs():
    bdma = _lib.query("bgnn_get_tuning", KNOB_BDMA)
    cstore = _lib.query("bgnn_get_tuning", KNOB_CSTORE)
    yield
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, 2)
    _lib.call("bgnn_set_tuning", KNOB_BDMA, bdma)
    _lib.call("bgnn_set_tuning", KNOB_CSTORE, cstore)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the row-segment epilogue tests, session ended: {e}", returncode=3)


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Win:
    """The M x N window, ldc = N + PAD, GUARD_ROWS rows of the pattern above and below."""

    def __init__(self, dev, M, N):
        self.M, self.N, self.ldc = M, N, N + PAD
        self.off = GUARD_ROWS * self.ldc + 4          # 16-B aligned (N % 4 == 0)
        self.buf = torch.empty((M + 2 * GUARD_ROWS) * self.ldc + 8, dtype=torch.float32, device=dev)
        self.ptr = self.buf.data_ptr() + 4 * self.off

    def view(self):
        return torch.as_strided(self.buf, (self.M, self.N), (self.ldc, 1), self.off)

    def fill(self, c0=None):
        self.buf.view(torch.int32).fill_(PATTERN)
        self.view().copy_(torch.full((self.M, self.N), float("nan")) if c0 is None else c0)

    def read(self):
        return self.view().cpu()

    def assert_guard(self, label):
        g = self.buf.view(torch.int32).clone()
        torch.as_strided(g, (self.M, self.N), (self.ldc, 1), self.off).fill_(PATTERN)
        bad = (g != PATTERN).nonzero().flatten()
        assert bad.numel() == 0, (f"{label}: {bad.numel()} elements outside the {self.M} x {self.N} window "
                                  f"overwritten; first at flat offset {int(bad[0])} (window at {self.off}, "
                                  f"ldc {self.ldc})")


def assert_close(out, ref, mag, label):
    assert bool(torch.isfinite(out).all()), f"{label}: window elements not finite (never written?)"
    err = (out.double() - ref).abs()
    bound = REL * mag + TINY
    over = err - bound
    worst = int(over.argmax())
    r, c = divmod(worst, out.size(1))
    print(f"{label}: max err/bound {float((err / bound).max()):.3f}")
    assert not bool((over > 0).any()), (f"{label}: {int((over > 0).sum())} elements over the bound; worst at "
                                        f"({r}, {c}): |err| {err[r, c].item():.3g} > {bound[r, c].item():.3g}")


def operands(dev, M, N, K, seed):
    g = gen(seed)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) * 0.05
    am = torch.tensor([a.abs().max().item(), w.abs().max().item()], dtype=torch.float32, device=dev)
    return g, a, w, a.to(dev), w.to(dev), am


def both_shapes(dev, M, N, label, launch, ref, mag, c0=None, cm0=None):
    """launch(win, cm) under knob 17 = 0 and 1: guard and fp64 for each, then bit identity."""
    outs, cms = [], []
    for shape in (0, 1):
        _lib.call("bgnn_set_tuning", KNOB_CSTORE, shape)
        win = Win(dev, M, N)
        win.fill(c0)
        cm = None if cm0 is None else torch.tensor([cm0], dtype=torch.float32, device=dev)
        launch(win, cm)
        torch.cuda.synchronize()
        out = win.read()
        win.assert_guard(f"{label} store shape {shape}")
        assert_close(out, ref, mag, f"{label} store shape {shape}")
        outs.append(out)
        if cm is not None:
            want = max(torch.tensor(cm0, dtype=torch.float32).item(), out.abs().max().item())
            assert cm.item() == want, f"{label} store shape {shape}: c_amax {cm.item()!r}, want {want!r}"
            cms.append(cm.item())
    assert torch.equal(outs[0], outs[1]), (f"{label}: the two store shapes differ in "
                                           f"{int((outs[0] != outs[1]).sum())} elements")
    if cms:
        assert cms[0] == cms[1], f"{label}: c_amax differs between the store shapes: {cms}"


def wsplit(dev, w_dev, N, K, am, bn):
    img = torch.empty(_lib.query("bgnn_gemm_wsplit_bytes", N, K), dtype=torch.uint8, device=dev)
    _lib.call("bgnn_gemm_wsplit", w_dev.data_ptr(), 1, 0, N, K, K, am[1:2].data_ptr(), 0, img.data_ptr(), img.numel(),
              bn, _stream())
    return img


def drop_of(dev, src, p):
    out = torch.empty_like(src)
    _lib.call("bgnn_add_dropout", src.data_ptr(), None, src.numel(), p, SEED, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu()


def select_h3(cfg, bdma):
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, 2)
    _lib.call("bgnn_gemm_set_cfg", cfg)
    _lib.call("bgnn_set_tuning", KNOB_BDMA, bdma)


@pytest.mark.parametrize("act", [False, True], ids=["plain", "bias-relu-amax"])
def test_forward_presplit_256(dev, act):
    """bgnn_gemm_f32_w on the 256 x 256 tile (4 x 2 waves of 64 x 128: 512-B segments): two interior
    row tiles plus a ragged one on the general path, two column tiles, two k-steps."""
    M, N, K = 256 + 256 + 37, 512, 64
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 11)
    select_h3(4, 3)
    bn = _lib.query("bgnn_gemm_w_tile", M, N, K)
    assert bn == 256, f"the 256 x 256 tile is no longer planned for the pre-split path (tile {bn})"
    img = wsplit(dev, w_dev, N, K, am, bn)
    ref, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    bias = None
    if act:
        bv = torch.randn(N, generator=g)
        bias = bv.to(dev)
        ref, mag = (ref + bv.double()).clamp_min(0), mag + bv.double().abs()

    def launch(win, cm):
        _lib.call("bgnn_gemm_f32_w", M, N, K, a_dev.data_ptr(), K, img.data_ptr(), bn, win.ptr, win.ldc,
                  bias.data_ptr() if act else None, int(act), am[0:1].data_ptr(), am[1:2].data_ptr(),
                  cm.data_ptr() if cm is not None else None, None, 0, 0.0, 0, _stream())

    both_shapes(dev, M, N, f"fwd f32_w 256x256 act={act}", launch, ref, mag,
                cm0=0.25 * float(ref.abs().max()) if act else None)


@pytest.mark.parametrize("bdma", [2, 3, 0], ids=["h3p-3slots", "h3p-4slots", "x6"])
@pytest.mark.parametrize("p", [None, 0.0, 0.1], ids=["plain", "dropadd-p0", "dropadd-p0.1"])
def test_dgrad_tile_128x256(dev, p, bdma):
    """The 128 x 256 tile (2 x 4 waves of 64 x 64: 256-B segments), M = 2 tiles + 5 rows, K = 128
    (4 k-steps >= the B slots): the pipelined kernel plain and with its LDS-source drop-add epilogue
    (knob 16 = 2 / 3), and k_gemm_x6 with the prefetched source rows (knob 16 = 0)."""
    M, N, K = 128 * 2 + 5, 512, 128
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 12)
    select_h3(2, bdma)
    bn = _lib.query("bgnn_gemm_w_tile", M, N, K)
    assert bn == 256
    img = wsplit(dev, w_dev, N, K, am, bn)
    ref, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    src = None
    if p is not None:
        src = torch.randn(M, N, generator=g).to(dev)
        drop = drop_of(dev, src, p).double()
        assert p == 0.0 or (bool((drop == 0).any()) and not bool((drop == 0).all()))
        ref, mag = ref + drop, mag + drop.abs()

    def launch(win, cm):
        _lib.call("bgnn_gemm_f32_w", M, N, K, a_dev.data_ptr(), K, img.data_ptr(), bn, win.ptr, win.ldc, None, 0,
                  am[0:1].data_ptr(), am[1:2].data_ptr(), None, src.data_ptr() if src is not None else None, N,
                  p or 0.0, SEED, _stream())

    both_shapes(dev, M, N, f"128x256 f32_w knob16={bdma} p={p}", launch, ref, mag)


@pytest.mark.parametrize("p", [0.0, 0.1])
def test_dropadd_prefetch_256(dev, p):
    """bgnn_gemm_f32_dropadd on the 256 x 256 tile: the prefetched source rows (32 float4 per lane)."""
    M, N, K = 256 + 37, 512, 64
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 13)
    select_h3(4, 3)
    src = torch.randn(M, N, generator=g).to(dev)
    drop = drop_of(dev, src, p).double()
    ref, mag = a.double() @ w.double().t() + drop, a.double().abs() @ w.double().abs().t() + drop.abs()
    nws = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)

    def launch(win, cm):
        _lib.call("bgnn_gemm_f32_dropadd", 0, 1, M, N, K, a_dev.data_ptr(), K, w_dev.data_ptr(), K, win.ptr, win.ldc,
                  am[0:1].data_ptr(), am[1:2].data_ptr(), src.data_ptr(), N, p, SEED, ws.data_ptr(), nws, _stream())

    both_shapes(dev, M, N, f"dropadd 256x256 p={p}", launch, ref, mag)


# (tile config, M, N, K): 256 x 256 as 4 x 2 and 2 x 4 waves, 128 x 256, 256 x 128, and the tall
# 8-wave 128 x 128 tile (2 x 4 waves of 64 x 32: three row tiles, one column tile)
SCALED = [(4, 256 + 37, 512, 64), (3, 256 + 37, 512, 64), (2, 128 * 2 + 5, 512, 64), (1, 256 + 37, 256, 64),
          (5, 128 * 3, 128, 64)]


@pytest.mark.parametrize("cfg,M,N,K", SCALED, ids=[f"cfg{c[0]}" for c in SCALED])
def test_scaled_alpha_beta_bias_relu(dev, cfg, M, N, K):
    """alpha = 0.75, beta = -0.5 with C as the addend (read back as row segments), bias, ReLU, max|C|."""
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 14 + cfg)
    select_h3(cfg, 3)
    c0 = torch.randn(M, N, generator=g)
    bv = torch.randn(N, generator=g)
    bias = bv.to(dev)
    ref = 0.75 * (a.double() @ w.double().t()) - 0.5 * c0.double() + bv.double()
    mag = 0.75 * (a.double().abs() @ w.double().abs().t()) + 0.5 * c0.double().abs() + bv.double().abs()
    ref = ref.clamp_min(0)
    nws = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)

    def launch(win, cm):
        _lib.call("bgnn_gemm_f32_scaled", 0, 1, M, N, K, 0.75, a_dev.data_ptr(), K, 0, 0, w_dev.data_ptr(), K, -0.5,
                  win.ptr, win.ldc, 0, 0, bias.data_ptr(), 1, am[0:1].data_ptr(), am[1:2].data_ptr(), cm.data_ptr(),
                  0, ws.data_ptr(), nws, _stream())

    both_shapes(dev, M, N, f"scaled cfg {cfg} M={M} N={N} K={K}", launch, ref, mag, c0=c0,
                cm0=0.25 * float(ref.abs().max()))


@pytest.mark.parametrize("cfg,M,N,K", SCALED, ids=[f"cfg{c[0]}" for c in SCALED])
def test_scaled_plain(dev, cfg, M, N, K):
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 24 + cfg)
    select_h3(cfg, 3)
    ref, mag = a.double() @ w.double().t(), a.double().abs() @ w.double().abs().t()
    nws = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0)
    ws = torch.empty(max(nws, 256), dtype=torch.uint8, device=dev)

    def launch(win, cm):
        _lib.call("bgnn_gemm_f32_scaled", 0, 1, M, N, K, 1.0, a_dev.data_ptr(), K, 0, 0, w_dev.data_ptr(), K, 0.0,
                  win.ptr, win.ldc, 0, 0, None, 0, am[0:1].data_ptr(), am[1:2].data_ptr(), None, 0, ws.data_ptr(), nws,
                  _stream())

    both_shapes(dev, M, N, f"scaled plain cfg {cfg} M={M} N={N} K={K}", launch, ref, mag)


@pytest.mark.parametrize("cfg", [4, 2])
def test_gather_add(dev, cfg):
    """act(A B^T + bias + add0[idx0] + add1[idx1]) on an f16x3 config: the gathered rows follow the new walk."""
    bm = 256 if cfg == 4 else 128
    M, N, K, R = bm + 37, 512, 64, 41
    g, a, w, a_dev, w_dev, am = operands(dev, M, N, K, 34 + cfg)
    select_h3(cfg, 3)
    idx = [torch.randint(0, R, (M,), generator=g) for _ in range(2)]
    idx[0][0], idx[0][-1], idx[1][0], idx[1][-1] = 0, R - 1, R - 1, 0
    adds = [torch.randn(R, N, generator=g) for _ in range(2)]
    bv = torch.randn(N, generator=g)
    gathered = adds[0][idx[0]].double() + adds[1][idx[1]].double()
    ref = (a.double() @ w.double().t() + gathered + bv.double()).clamp_min(0)
    mag = (a.double().abs() @ w.double().abs().t() + adds[0][idx[0]].double().abs() + adds[1][idx[1]].double().abs() +
           bv.double().abs())
    bias, adds_dev, idx_dev = bv.to(dev), [x.to(dev) for x in adds], [i.to(dev) for i in idx]
    nws = max(_lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0), 256)
    ws = torch.empty(nws, dtype=torch.uint8, device=dev)

    def launch(win, cm):
        _lib.call("bgnn_gemm_gather_add", 0, 1, M, N, K, a_dev.data_ptr(), K, w_dev.data_ptr(), K, win.ptr, win.ldc,
                  bias.data_ptr(), 1, adds_dev[0].data_ptr(), idx_dev[0].data_ptr(), N, adds_dev[1].data_ptr(),
                  idx_dev[1].data_ptr(), N, 0, ws.data_ptr(), nws, _stream())

    both_shapes(dev, M, N, f"gather_add cfg {cfg}", launch, ref, mag)
