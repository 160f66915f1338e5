"""GPU: small-shape fp64 conformance matrix of the GEMM -- every tile config of the three kernel
families (f32 MFMA, f16x3, bf16-operand) on every epilogue path, each case against an fp64
reference per element and with a sentinel around the output window.

Every case: operands drawn on the CPU, an fp64 reference and magnitude from the same f32 values
(bf16 family: from the bf16-rounded values), the bound |c - ref| <= 2e-6 * mag + TINY with
mag = |alpha| |A||B| + |beta| |C0| + |bias| + |drop(src)| + |gathered rows|. The output is a window
inside a larger buffer (>= 2 guard rows above and below, >= 5 guard columns left and right within
ldc, the gap between C planes, the bytes after a split-K workspace): the window starts as NaN
(beta == 0) or a known C0, everything else holds a fixed bit pattern that must survive the call.
Operand buffers carry NaN in their row padding, so a read past K / M / N poisons the result.

Sections: A tile x transpose, B epilogue options and alignments with max|C|, C plane-split
operands on forced tiles, D split-K (float4 / scalar / two-stage reduce, workspace fallback),
E drop-add epilogues against bgnn_add_dropout + fp64, F gather-add epilogue.
A failure message names family, config, transposes, shape and path."""
import pytest
import torch

from bgnn import _lib, fused
from bgnn.graph import _stream

pytestmark = pytest.mark.gpu

TINY = 1e-37            # denormal-scale floor of the bound
REL = 2e-6              # tests/test_gpu_gemm.py's per-element class
PATTERN = 0x4B1D5EED    # guard bit pattern (as f32: 1.03e7, finite -- a read of it as C0 shows too)
WS_FILL = 0xA5

# (bm, bn) per config index; mirrors kCfgs in csrc/gemm.hip ...
F32_TILES = [(128, 128), (256, 256), (256, 256), (256, 128), (256, 128), (128, 256), (128, 256), (256, 256),
             (256, 128)]
# ... and kX6Cfgs in csrc/gemm_x6.hip (config 5: f16x3 C = A B^T only)
X6_TILES = [(128, 128), (256, 128), (128, 256), (256, 256), (256, 256), (128, 128)]

# family -> (BGNN_TUNE_GEMM_MODE, precision argument, tiles, workspace head bytes)
FAMS = {
    "f32": (0, 0, F32_TILES, 0),
    "h3": (2, 0, X6_TILES, 256),
    "bf16": (2, 1, X6_TILES[:5], 0),
}
ALL_CFGS = [(f, c) for f in FAMS for c in range(len(FAMS[f][2]))]
TRANSPOSES = [(0, 0), (0, 1), (1, 0), (1, 1)]

REMAP_H3_5 = "the planner remaps a forced f16x3 config 5 to config 1 (256 x 128) outside C = A B^T"
REMAP_BF16_5 = "the planner remaps bf16 config 5 to config 1 (256 x 128): the 8-wave 128 x 128 tile is f16x3 only"


def remapped(fam, cfg, ta, tb):
    if fam == "h3" and cfg == 5 and (ta, tb) != (0, 1):
        return REMAP_H3_5
    return None


def shape_of(variant, bm, bn):
    if variant == "unal":     # 2 x 2 tiles, three ragged edges, N % 4 == 2, K no multiple of any BK
        return bm + 37, bn + 22, 79
    if variant == "al":       # fast interior tile + vectorised general-path edge tiles
        return bm + 40, bn + 36, 96
    if variant == "t9":       # 3 x 3 tiles: a tile count the 8 XCDs do not divide
        return 2 * bm + 8, 2 * bn + 4, 32
    raise ValueError(variant)


_DEFAULT_BDMA = None


@pytest.fixture(autouse=True)
def _restore_knobs():
    global _DEFAULT_BDMA
    if _DEFAULT_BDMA is None:
        _DEFAULT_BDMA = _lib.query("bgnn_get_tuning", 16)
    yield
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, 2)
    _lib.call("bgnn_set_tuning", 16, _DEFAULT_BDMA)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the GEMM matrix, session ended: {e}", returncode=3)


def select(fam, cfg):
    """Kernel family, then the forced tile (-1 = planned): the cfg range depends on the mode."""
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, FAMS[fam][0])
    _lib.call("bgnn_gemm_set_cfg", cfg)


def ceil4(x):
    return (x + 3) // 4 * 4


def gen(seed):
    return torch.Generator().manual_seed(seed)


class Win:
    """The M x N output window inside a guarded flat buffer; c_blk > 0: plane-split along N
    (planes of c_blk columns, c_pstride elements apart, each with its own guard rows / columns)."""

    def __init__(self, dev, M, N, place="al", c_blk=0):
        width = c_blk if c_blk else N
        co, ldc = {"al": (8, ceil4(width + 16)), "off1": (9, ceil4(width + 20)),
                   "odd": (8, ceil4(width + 16) + 1)}[place]
        planes = (N + c_blk - 1) // c_blk if c_blk else 1
        pstride = (M + 4) * ldc + (9 if place == "odd" else 8)
        off = 2 * ldc + co
        r = torch.arange(M).view(M, 1)
        c = torch.arange(N).view(1, N)
        idx = off + r * ldc + ((c // c_blk) * pstride + c % c_blk if c_blk else c)
        self.M, self.N, self.ldc, self.c_blk = M, N, ldc, c_blk
        self.c_pstride = pstride if c_blk else 0
        self.idx = idx.to(dev)
        self.buf = torch.empty(planes * pstride, dtype=torch.float32, device=dev)
        self.ptr = self.buf.data_ptr() + 4 * off

    def fill(self, c0=None):
        self.buf.view(torch.int32).fill_(PATTERN)
        self.buf[self.idx] = float("nan") if c0 is None else c0.to(self.buf.device)

    def read(self):
        return self.buf[self.idx].cpu()

    def view2d(self):
        """The dense window as a strided [M, N] tensor (fused.gemm's out)."""
        assert not self.c_blk
        return torch.as_strided(self.buf, (self.M, self.N), (self.ldc, 1), (self.ptr - self.buf.data_ptr()) // 4)

    def assert_guard(self, label):
        g = self.buf.view(torch.int32).clone()
        g[self.idx] = PATTERN
        bad = (g != PATTERN).nonzero().flatten()
        assert bad.numel() == 0, (f"{label}: {bad.numel()} guard elements outside the {self.M} x {self.N} window "
                                  f"overwritten; first at flat offset {int(bad[0])} (ldc {self.ldc}, window at "
                                  f"{(self.ptr - self.buf.data_ptr()) // 4}, c_blk {self.c_blk}, "
                                  f"c_pstride {self.c_pstride})")


class Ws:
    """Workspace of `nbytes` followed by a guard."""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 256,), WS_FILL, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() if nbytes else None

    def assert_guard(self, label):
        assert bool((self.buf[self.nbytes:] == WS_FILL).all()), \
            f"{label}: bytes after the {self.nbytes}-byte workspace overwritten"


def operand(dev, rows, cols, g, aligned=True, scale=1.0):
    """randn [rows, cols] in a row-padded device buffer whose padding is NaN. Returns (cpu values,
    device buffer, ld); aligned: ld % 4 == 0 (vector loads), else ld % 4 != 0."""
    v = torch.randn(rows, cols, generator=g) * scale
    ld = ceil4(cols) + 4 if aligned else cols + (5 if (cols + 5) % 4 else 6)
    buf = torch.full((rows, ld), float("nan"))
    buf[:, :cols] = v
    return v, buf.to(dev), ld


def planes_operand(dev, v, blk):
    """[rows, cols] values as planes of blk columns: tensor [P, rows, blk], NaN past cols."""
    rows, cols = v.shape
    P = (cols + blk - 1) // blk
    buf = torch.full((P, rows, blk), float("nan"))
    for p in range(P):
        w = min(blk, cols - p * blk)
        buf[p, :, :w] = v[:, p * blk:p * blk + w]
    return buf.to(dev), blk, (blk if P > 1 else 0), rows * blk


def product(a, b, ta, tb, bf16):
    """fp64 op(A) op(B) and |op(A)| |op(B)| of the f32 (bf16 family: bf16-rounded) operands."""
    A = (a.bfloat16() if bf16 else a).double()
    B = (b.bfloat16() if bf16 else b).double()
    A = A.t() if ta else A
    B = B.t() if tb else B
    return A @ B, A.abs() @ B.abs()


def assert_close(out, ref, mag, label):
    fin = torch.isfinite(out)
    if not bool(fin.all()):
        r, c = (~fin).nonzero()[0].tolist()
        raise AssertionError(f"{label}: {int((~fin).sum())} window elements not finite (never written, or a read "
                             f"past an operand edge); first at ({r}, {c})")
    err = (out.double() - ref).abs()
    bound = REL * mag + TINY
    over = err - bound
    if bool((over > 0).any()):
        i = int(over.argmax())
        r, c = divmod(i, out.size(1))
        raise AssertionError(f"{label}: {int((over > 0).sum())} elements over the bound; worst at ({r}, {c}): "
                             f"got {out[r, c].item():.9g}, fp64 {ref[r, c].item():.9g}, |err| {err[r, c].item():.3g} "
                             f"> {bound[r, c].item():.3g} (mag {mag[r, c].item():.3g})")


def run_case(dev, fam, cfg, ta, tb, M, N, K, *, alpha=1.0, beta=0.0, bias=None, relu=False, place="al",
             c_blk=0, a_planes=False, amax=None, ws_mode="full", expect_split=0, twice=False, aligned_in=None,
             seed=0, via_fused=False, label=""):
    """One bgnn_gemm_f32_scaled (or fused.gemm) call on the selected family / tile, checked against
    fp64 per element, the sentinel, the workspace guard and (amax) the max|C| fold."""
    mode, prec, tiles, head = FAMS[fam]
    label = (f"{label} {fam} cfg {cfg} ta={ta} tb={tb} M={M} N={N} K={K} alpha={alpha} beta={beta} bias={bias} "
             f"relu={relu} C {place} c_blk={c_blk} a_planes={a_planes} amax={amax} ws={ws_mode}")
    select(fam, cfg)
    g = gen(seed + 1000 * M + 10 * N + K)
    if aligned_in is None:
        aligned_in = M % 4 == 0 and N % 4 == 0 and K % 4 == 0
    a, a_dev, lda = operand(dev, K if ta else M, M if ta else K, g, aligned_in)
    b, b_dev, ldb = operand(dev, N if tb else K, K if tb else N, g, aligned_in)
    a_blk = a_ps = 0
    if a_planes:   # planes cut A's contiguous dimension: K (ta = 0, 32 wide) or M (ta = 1, bm wide)
        a_dev, lda, a_blk, a_ps = planes_operand(dev, a, tiles[cfg][0] if ta else 32)
    ref, mag = product(a, b, ta, tb, fam == "bf16")
    ref, mag = alpha * ref, abs(alpha) * mag
    win = Win(dev, M, N, place, c_blk)
    c0 = None
    if beta != 0.0:
        c0 = torch.randn(M, N, generator=g)
        ref, mag = ref + beta * c0.double(), mag + abs(beta) * c0.double().abs()
    bias_ptr = None
    if bias is not None:
        bv = torch.randn(N, generator=g)
        bbuf = torch.full((N + 8,), float("nan"))
        o = 0 if bias == "al" else 1
        bbuf[o:o + N] = bv
        bbuf = bbuf.to(dev)
        bias_ptr = bbuf.data_ptr() + 4 * o
        ref, mag = ref + bv.double(), mag + bv.double().abs()
    if relu:
        ref = ref.clamp_min(0)
    cm = None
    if amax is not None:   # starts below / above the result's max |C|
        cm0 = float(ref.abs().max()) * (0.25 if amax == "lo" else 4.0) + (0.0 if amax == "lo" else 1.0)
        cm = torch.tensor([cm0], dtype=torch.float32, device=dev)
        cm0 = cm.item()
    ws_full = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, ta, tb, prec)
    if expect_split:   # split-K really planned (else this case silently tests split = 1)
        assert _lib.query("bgnn_gemm_ws_bytes", M, N, K, ta, tb) >= head + expect_split * M * N * 4, \
            f"{label}: the planner no longer splits K by {expect_split}"
    ws = Ws(dev, ws_full if ws_mode == "full" else head)
    outs = []
    for _ in range(2 if twice else 1):
        win.fill(c0)
        if via_fused:
            fused.gemm(a_dev[:, :a.size(1)], b_dev[:, :b.size(1)], bool(ta), bool(tb), out=win.view2d(),
                       bf16=bool(prec))
        else:
            _lib.call("bgnn_gemm_f32_scaled", ta, tb, M, N, K, alpha, a_dev.data_ptr(), lda, a_blk, a_ps,
                      b_dev.data_ptr(), ldb, beta, win.ptr, win.ldc, win.c_blk, win.c_pstride, bias_ptr, int(relu),
                      None, None, None if cm is None else cm.data_ptr(), prec, ws.ptr, ws.nbytes, _stream())
        torch.cuda.synchronize()
        out = win.read()
        assert_close(out, ref, mag, label)
        win.assert_guard(label)
        ws.assert_guard(label)
        if cm is not None and not outs:
            want = max(cm0, out.abs().max().item())
            assert cm.item() == want, f"{label}: c_amax {cm.item()!r}, want max(initial {cm0!r}, max|C|) = {want!r}"
        outs.append(out)
    if twice:
        assert torch.equal(outs[0], outs[1]), f"{label}: two calls differ in bits"
    return outs[0]


# ---------------------------------------------------------------------------------------------
# A. tile x transpose


def _a_params():
    ps = []
    for fam, cfg in ALL_CFGS + [("bf16", 5)]:
        for ta, tb in TRANSPOSES:
            for variant in ("unal", "al"):
                why = REMAP_BF16_5 if (fam, cfg) == ("bf16", 5) else remapped(fam, cfg, ta, tb)
                ps.append(pytest.param(fam, cfg, ta, tb, variant, id=f"{fam}-cfg{cfg}-ta{ta}tb{tb}-{variant}",
                                       marks=[pytest.mark.skip(reason=why)] if why else []))
    return ps


@pytest.mark.parametrize("fam,cfg,ta,tb,variant", _a_params())
def test_a_tile_transpose(dev, fam, cfg, ta, tb, variant):
    bm, bn = FAMS[fam][2][cfg]
    M, N, K = shape_of(variant, bm, bn)
    run_case(dev, fam, cfg, ta, tb, M, N, K, place="al" if variant == "al" else "off1", via_fused=True, label="A")


@pytest.mark.parametrize("fam,cfg", ALL_CFGS, ids=[f"{f}-cfg{c}" for f, c in ALL_CFGS])
def test_a_nine_tiles(dev, fam, cfg):
    """3 x 3 tiles: xcd_remap's uneven split; an unwritten or twice-mapped tile shows as NaN."""
    bm, bn = FAMS[fam][2][cfg]
    M, N, K = shape_of("t9", bm, bn)
    run_case(dev, fam, cfg, 0, 1, M, N, K, via_fused=True, label="A9")


# ---------------------------------------------------------------------------------------------
# B. epilogue matrix

# (C placement, bias base, initial c_amax): the fast interior path needs an aligned C and bias
B_COMBOS = [("al", "al", "lo"), ("al", "un", "hi"), ("off1", "al", "hi"), ("odd", "un", "lo")]


def _b_params():
    ps = []
    for fam, cfg in ALL_CFGS:
        for ta, tb in ((0, 1), (1, 0)):
            for variant in ("unal", "al"):
                why = remapped(fam, cfg, ta, tb)
                ps.append(pytest.param(fam, cfg, ta, tb, variant, id=f"{fam}-cfg{cfg}-ta{ta}tb{tb}-{variant}",
                                       marks=[pytest.mark.skip(reason=why)] if why else []))
    return ps


@pytest.mark.parametrize("fam,cfg,ta,tb,variant", _b_params())
def test_b_epilogue_all_options(dev, fam, cfg, ta, tb, variant):
    """alpha, beta, bias and ReLU together, max|C| folded (fused in the split families' epilogue,
    an extra pass in the f32 family), over C / bias alignments."""
    bm, bn = FAMS[fam][2][cfg]
    M, N, K = shape_of(variant, bm, bn)
    for place, bias, amax in B_COMBOS:
        run_case(dev, fam, cfg, ta, tb, M, N, K, alpha=0.75, beta=-0.5, bias=bias, relu=True, place=place,
                 amax=amax, seed=1, label="B")


# config 0 and the largest tile of each family
B_SINGLE_CFGS = [("f32", 0), ("f32", 1), ("h3", 0), ("h3", 3), ("h3", 4), ("bf16", 0), ("bf16", 3)]
B_SINGLE_OPTS = {"alpha": dict(alpha=0.75), "beta": dict(beta=-0.5), "bias": dict(bias="al"), "relu": dict(relu=True)}


@pytest.mark.parametrize("opt", list(B_SINGLE_OPTS))
@pytest.mark.parametrize("fam,cfg", B_SINGLE_CFGS, ids=[f"{f}-cfg{c}" for f, c in B_SINGLE_CFGS])
def test_b_epilogue_single_option(dev, fam, cfg, opt):
    bm, bn = FAMS[fam][2][cfg]
    for variant, place in (("al", "al"), ("unal", "off1")):
        M, N, K = shape_of(variant, bm, bn)
        for ta, tb in ((0, 1), (1, 0)):
            kw = dict(B_SINGLE_OPTS[opt])
            if opt == "bias" and place != "al":
                kw["bias"] = "un"
            run_case(dev, fam, cfg, ta, tb, M, N, K, place=place, amax="lo", seed=2, label=f"B1 {opt}", **kw)


# ---------------------------------------------------------------------------------------------
# C. plane-split operands on forced tiles


def _c_params():
    ps = []
    for fam, cfg in ALL_CFGS:
        for ta, tb in ((0, 1), (1, 0)):
            why = remapped(fam, cfg, ta, tb)
            ps.append(pytest.param(fam, cfg, ta, tb, id=f"{fam}-cfg{cfg}-ta{ta}tb{tb}",
                                   marks=[pytest.mark.skip(reason=why)] if why else []))
    return ps


@pytest.mark.parametrize("fam,cfg,ta,tb", _c_params())
def test_c_planes_forced_tiles(dev, fam, cfg, ta, tb):
    """Two C planes of c_blk = bn columns (the second one ragged; the gap between the planes is
    guarded) and A planes (32-wide along K for ta = 0, bm-wide along M for ta = 1), ragged M."""
    bm, bn = FAMS[fam][2][cfg]
    M, N, K = shape_of("al" if ta == 0 else "unal", bm, bn)
    run_case(dev, fam, cfg, ta, tb, M, N, K, c_blk=bn, a_planes=True, seed=3, label="C")
    run_case(dev, fam, cfg, ta, tb, M, N, K, alpha=0.75, beta=-0.5, bias="al", relu=True, c_blk=bn, a_planes=True,
             amax="lo", seed=3, label="C")


# ---------------------------------------------------------------------------------------------
# D. split-K on planned tiles

D_SHAPES = {"f4": (150, 132, 1041, 4), "scalar": (150, 131, 1041, 4), "stage2": (64, 48, 4200, 16)}


@pytest.mark.parametrize("ta,tb", [(1, 0), (0, 1)], ids=["tn", "nt"])
@pytest.mark.parametrize("shape", list(D_SHAPES))
@pytest.mark.parametrize("fam", ["f32", "h3"])
def test_d_split_k(dev, fam, shape, ta, tb):
    """float4 reduce (N % 4 == 0, aligned), scalar reduce (N % 4 != 0, or an unaligned C), two-stage
    reduce with an empty last K slice on the 32-deep family; each deterministic, each again through
    the split = 1 fallback of a workspace that holds no slab."""
    M, N, K, split = D_SHAPES[shape]
    opts = dict(alpha=0.75, beta=-0.5, bias="al", relu=True, amax="lo", seed=4)
    for ws_mode in ("full", "head"):
        kw = dict(opts, ws_mode=ws_mode, expect_split=split, aligned_in=True, label=f"D {shape}")
        run_case(dev, fam, -1, ta, tb, M, N, K, place="al", twice=ws_mode == "full", **kw)
        run_case(dev, fam, -1, ta, tb, M, N, K, place="off1", **dict(kw, bias="un", amax="hi"))
        run_case(dev, fam, -1, ta, tb, M, N, K, place="al", **dict(kw, alpha=1.0, beta=0.0, bias=None, relu=False))
        if shape == "f4":   # two C planes: 128 columns and the 4 left over
            run_case(dev, fam, -1, ta, tb, M, N, K, place="al", c_blk=128, **kw)


# ---------------------------------------------------------------------------------------------
# E. drop-add epilogues against bgnn_add_dropout + fp64 (f16x3, C = A W^T)

SEED = 1234


def drop_of(dev, src, p, seed):
    """drop(src) over the whole padded [M, ld_src] buffer by bgnn_add_dropout (mask by flat index / 4)."""
    out = torch.empty_like(src)
    _lib.call("bgnn_add_dropout", src.data_ptr(), None, src.numel(), p, seed, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    return out.cpu()


def nt_operands(dev, M, N, K, g):
    a, a_dev, lda = operand(dev, M, K, g)
    w, w_dev, ldw = operand(dev, N, K, g, scale=0.05)
    am = torch.tensor([a.abs().max().item(), w.abs().max().item()], dtype=torch.float32, device=dev)
    return a, a_dev, lda, w, w_dev, ldw, am


def assert_tiles_mixed(dropped, bm, bn, label):
    """Every tile of the window holds both kept and dropped elements."""
    M, N = dropped.shape
    for r0 in range(0, M, bm):
        for c0 in range(0, N, bn):
            t = dropped[r0:r0 + bm, c0:c0 + bn]
            assert bool(t.any()) and not bool(t.all()), f"{label}: tile at ({r0}, {c0}) is not mixed"


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("pad", [0, 12], ids=["ldN", "ldN+12"])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2, 3, 4, 5])
def test_e_dropadd(dev, cfg, pad, p):
    bm, bn = X6_TILES[max(cfg, 0)]
    M, N, K = shape_of("al", bm, bn)
    ld_src = N + pad
    g = gen(50 + cfg)
    a, a_dev, lda, w, w_dev, ldw, am = nt_operands(dev, M, N, K, g)
    src = torch.randn(M, ld_src, generator=g).to(dev)
    drop = drop_of(dev, src, p, SEED)[:, :N]
    prod, mag = product(a, w, 0, 1, False)
    ref, mag = prod + drop.double(), mag + drop.double().abs()
    dropped = drop == 0
    if p > 0:
        assert_tiles_mixed(dropped, bm, bn, f"E p={p}")
    else:
        assert torch.equal(drop, src[:, :N].cpu())
    select("h3", cfg)
    ws = Ws(dev, _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0))
    for place in ("al", "off1"):
        label = f"E dropadd h3 cfg {cfg} M={M} N={N} K={K} ld_src={ld_src} p={p} C {place}"
        win = Win(dev, M, N, place)
        win.fill()
        _lib.call("bgnn_gemm_f32_dropadd", 0, 1, M, N, K, a_dev.data_ptr(), lda, w_dev.data_ptr(), ldw, win.ptr,
                  win.ldc, am[0:1].data_ptr(), am[1:2].data_ptr(), src.data_ptr(), ld_src, p, SEED, ws.ptr, ws.nbytes,
                  _stream())
        torch.cuda.synchronize()
        out = win.read()
        assert_close(out, ref, mag, label)
        win.assert_guard(label)
        ws.assert_guard(label)
        if p > 0:   # a dropped element is exactly the plain product of the same tile and maxima
            plain = Win(dev, M, N, place)
            plain.fill()
            _lib.call("bgnn_gemm_f32_scaled", 0, 1, M, N, K, 1.0, a_dev.data_ptr(), lda, 0, 0, w_dev.data_ptr(), ldw,
                      0.0, plain.ptr, plain.ldc, 0, 0, None, 0, am[0:1].data_ptr(), am[1:2].data_ptr(), None, 0,
                      ws.ptr, ws.nbytes, _stream())
            torch.cuda.synchronize()
            pl = plain.read()
            assert torch.equal(out[dropped], pl[dropped]), f"{label}: dropped elements differ from the plain product"


@pytest.mark.parametrize("pad", [0, 12], ids=["ldC", "ldC+12"])
@pytest.mark.parametrize("cfg", [-1, 0, 1, 2])
def test_e_dropadd_cols(dev, cfg, pad):
    """[A Wl^T | A Wr^T + drop(src)]: the left block is the plain product, the right block adds the
    masked source under src's own flat indices (row * ld_src + col - src_col0)."""
    bm, bn = X6_TILES[max(cfg, 0)]
    M, N, K, c0, p = bm + 40, 2 * bn, 96, bn, 0.1
    ld_src = bn + pad
    g = gen(60 + cfg)
    a, a_dev, lda, w, w_dev, ldw, am = nt_operands(dev, M, N, K, g)
    src = torch.randn(M, ld_src, generator=g).to(dev)
    drop = drop_of(dev, src, p, SEED)[:, :bn]
    assert_tiles_mixed(drop == 0, bm, bn, "E cols")
    ref, mag = product(a, w, 0, 1, False)
    ref[:, c0:] += drop.double()
    mag[:, c0:] += drop.double().abs()
    select("h3", cfg)
    ws = Ws(dev, _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, 0))
    for place in ("al", "off1"):
        label = f"E dropadd_cols h3 cfg {cfg} M={M} N={N} K={K} src_col0={c0} ld_src={ld_src} C {place}"
        win = Win(dev, M, N, place)
        win.fill()
        _lib.call("bgnn_gemm_f32_dropadd_cols", M, N, K, a_dev.data_ptr(), lda, w_dev.data_ptr(), ldw, win.ptr,
                  win.ldc, am[0:1].data_ptr(), am[1:2].data_ptr(), src.data_ptr(), ld_src, c0, p, SEED, ws.ptr,
                  ws.nbytes, _stream())
        torch.cuda.synchronize()
        out = win.read()
        assert_close(out[:, :c0], ref[:, :c0], mag[:, :c0], label + " left block")
        assert_close(out[:, c0:], ref[:, c0:], mag[:, c0:], label + " right block")
        win.assert_guard(label)
        ws.assert_guard(label)


@pytest.mark.parametrize("K", [32, 128])
@pytest.mark.parametrize("ntile", [1, 2])
@pytest.mark.parametrize("bdma", [0, 2, 3])
@pytest.mark.parametrize("cfg", [1, 2, 3, 4])
def test_e_presplit_weights(dev, cfg, bdma, ntile, K):
    """bgnn_gemm_wsplit + bgnn_gemm_f32_w against fp64 (not against the sibling kernel): the plain
    epilogue with bias, ReLU and max|C|, and the drop-add epilogue, for every B staging of knob 16."""
    bm, bn = X6_TILES[cfg]
    M, N, p = bm + 40, ntile * bn, 0.1
    g = gen(70 + cfg)
    a, a_dev, lda, w, w_dev, ldw, am = nt_operands(dev, M, N, K, g)
    select("h3", cfg)
    _lib.call("bgnn_set_tuning", 16, bdma)
    tile = _lib.query("bgnn_gemm_w_tile", M, N, K)
    if tile == 0:
        pytest.skip(f"no pre-split path for (M, N, K) = ({M}, {N}, {K}) on config {cfg}")
    assert tile == bn
    img = Ws(dev, _lib.query("bgnn_gemm_wsplit_bytes", N, K))
    _lib.call("bgnn_gemm_wsplit", w_dev.data_ptr(), 1, 0, N, K, ldw, am[1:2].data_ptr(), 0, img.ptr, img.nbytes, bn,
              _stream())
    prod, pmag = product(a, w, 0, 1, False)
    bv = torch.randn(N, generator=g)
    bias = bv.to(dev)
    srcs = []   # (source, ld_src, drop(source)) with ld_src = N and N + 12
    for pad in (0, 12):
        src = torch.randn(M, N + pad, generator=g).to(dev)
        srcs.append((src, N + pad, drop_of(dev, src, p, SEED)[:, :N].double()))
    for place in ("al", "off1"):
        label = f"E f32_w h3 cfg {cfg} knob16={bdma} M={M} N={N} K={K} C {place}"
        # plain epilogue
        ref, mag = (prod + bv.double()).clamp_min(0), pmag + bv.double().abs()
        cm0 = 0.25 * float(ref.abs().max())
        cm = torch.tensor([cm0], dtype=torch.float32, device=dev)
        cm0 = cm.item()
        win = Win(dev, M, N, place)
        win.fill()
        _lib.call("bgnn_gemm_f32_w", M, N, K, a_dev.data_ptr(), lda, img.ptr, bn, win.ptr, win.ldc, bias.data_ptr(), 1,
                  am[0:1].data_ptr(), am[1:2].data_ptr(), cm.data_ptr(), None, 0, 0.0, 0, _stream())
        torch.cuda.synchronize()
        out = win.read()
        assert_close(out, ref, mag, label + " plain")
        win.assert_guard(label + " plain")
        assert cm.item() == max(cm0, out.abs().max().item()), f"{label}: c_amax {cm.item()!r}"
        # drop-add epilogue
        for src, ld_src, drop in srcs:
            win.fill()
            _lib.call("bgnn_gemm_f32_w", M, N, K, a_dev.data_ptr(), lda, img.ptr, bn, win.ptr, win.ldc, None, 0,
                      am[0:1].data_ptr(), am[1:2].data_ptr(), None, src.data_ptr(), ld_src, p, SEED, _stream())
            torch.cuda.synchronize()
            assert_close(win.read(), prod + drop, pmag + drop.abs(), f"{label} drop-add ld_src={ld_src}")
            win.assert_guard(f"{label} drop-add ld_src={ld_src}")
    img.assert_guard("wsplit image")


# ---------------------------------------------------------------------------------------------
# F. gather-add epilogue


@pytest.mark.parametrize("variant", ["unal", "al"])
@pytest.mark.parametrize("cfg", [0, 1, 2, 3, 4])
@pytest.mark.parametrize("prec", [0, 1], ids=["h3", "bf16"])
def test_f_gather_add(dev, prec, cfg, variant):
    """act(A B^T + bias + add0[idx0] + add1[idx1]): index vectors that repeat rows and hold the
    first and the last row; addends with aligned rows (ld = N) and the scalar branch (ld = N + 3,
    offset base); with and without bias + ReLU."""
    fam = "bf16" if prec else "h3"
    bm, bn = X6_TILES[cfg]
    M, N, K = shape_of(variant, bm, bn)
    R = 41
    g = gen(80 + cfg)
    a, a_dev, lda = operand(dev, M, K, g, variant == "al")
    b, b_dev, ldb = operand(dev, N, K, g, variant == "al")
    prod, pmag = product(a, b, 0, 1, bool(prec))
    idx = [torch.randint(0, R, (M,), generator=g) for _ in range(2)]
    idx[0][0], idx[0][-1], idx[1][0], idx[1][-1] = 0, R - 1, R - 1, 0
    bv = torch.randn(N, generator=g)
    bias = bv.to(dev)
    select(fam, cfg)
    ws = Ws(dev, max(_lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, 0, 1, prec), 256))
    for ld_pad, off in ((0, 0), (3, 1)):
        adds, bufs = [], []
        for _ in range(2):
            v = torch.randn(R, N, generator=g)
            buf = torch.full((R * (N + ld_pad) + 4,), float("nan"))
            buf[off:off + R * (N + ld_pad)].view(R, N + ld_pad)[:, :N] = v
            adds.append(v)
            bufs.append(buf.to(dev))
        gathered = adds[0][idx[0]].double() + adds[1][idx[1]].double()
        gmag = adds[0][idx[0]].double().abs() + adds[1][idx[1]].double().abs()
        idx_dev = [i.to(dev) for i in idx]
        for act in (False, True):
            label = f"F gather_add {fam} cfg {cfg} M={M} N={N} K={K} ld0={N + ld_pad} base+{off} bias/relu={act}"
            ref, mag = prod + gathered, pmag + gmag
            if act:
                ref, mag = (ref + bv.double()).clamp_min(0), mag + bv.double().abs()
            for place in ("al", "off1"):
                win = Win(dev, M, N, place)
                win.fill()
                _lib.call("bgnn_gemm_gather_add", 0, 1, M, N, K, a_dev.data_ptr(), lda, b_dev.data_ptr(), ldb, win.ptr,
                          win.ldc, bias.data_ptr() if act else None, int(act), bufs[0].data_ptr() + 4 * off,
                          idx_dev[0].data_ptr(), N + ld_pad, bufs[1].data_ptr() + 4 * off, idx_dev[1].data_ptr(),
                          N + ld_pad, prec, ws.ptr, ws.nbytes, _stream())
                torch.cuda.synchronize()
                assert_close(win.read(), ref, mag, f"{label} C {place}")
                win.assert_guard(f"{label} C {place}")
                ws.assert_guard(label)
