"""GPU: small-shape fp64 conformance matrix of the bf16-STORAGE GEMM family and the bf16 helpers of
csrc/elem.hip, every kernel on its raw entry point.

References, bounds, inputs and case lists: tests/gemm_b16_ref.py (tests/test_gemm_b16_ref.py shows on
the CPU that the bounds have teeth). Every output is a NaN window inside a guarded allocation (the
GEMM matrix's bit pattern 0x4B1D5EED, at least two guard rows above and below, the ld padding; a bf16
window is compared as 16-bit words); operand buffers carry bf16 / f32 NaN in their row padding, before
their first and after their last row; gather tables have NaN rows beyond the largest index.

Sections (the branch a case is there for is in its id or in the comment next to the case list):
  A  the LDS-DMA kernel k_gemm_b16<256,256,64,2,2,4,C16,1,true>, plain: bgnn_gemm_bf16 NT storage 3 / 7.
     Epilogue routes per wave (128 rows x 64 columns): whole-line bf16 walk (bf16 C, the wave's 64 columns
     inside N, aligned C / bias, ldc % 8 == 0; rows past M skipped one by one); 32-column block walk
     (f32 C, the same and all 128 rows inside M); x6_epilogue fall-back (edge column blocks, f32 C row
     edges, ldc % 8 != 0, C or bias off a 16-byte boundary).
  B  the same kernel gathered (bgnn_gemm_gather_add_bf16): the LDS copy of the gather indices
     (whole-line walk), the global indices (block walk, fall-back), unaligned tables (fall-back).
  C  the drop-add arm (bgnn_gemm_bf16_dropadd, st & 8) and its two-step forms.
  D  the register-staged storage kernels k_gemm_x6<2, ...>: every built (ta, tb, storage) on every
     forced tile; vector and element-guarded arms of x6_load<BF>, kq_load<BF>, kq_load16 / kq_store16;
     st_bf16x4 and scalar bf16 C stores; alpha / beta; split-K; K = 0 and 8; the rounding set.
  E  bgnn_add_dropout_bf16, bgnn_add_dropped_bf16, bgnn_segment_sum_bf16, bgnn_segment_bcast_bf16.
Exact cases compare bit for bit; random cases against the bounds of gemm_b16_ref.py."""
import pytest
import torch

import gemm_b16_ref as R
from bgnn import _lib
from bgnn.graph import _stream
from matrix_util import RATIOS, Buf, OutB16, Win, check, ptr

pytestmark = pytest.mark.gpu

D = torch.float64
BF, F32 = torch.bfloat16, torch.float32
WS_FILL = 0xA5


@pytest.fixture(autouse=True)
def _restore_knobs():
    yield
    _lib.call("bgnn_gemm_b16_variant", 0)
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, 2)
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the bf16-storage matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection 4d: largest err / bound")
    for k in sorted(RATIOS):
        if k.startswith("4d "):
            print(f"  {k}: {RATIOS[k]:.3f}")


def select(cfg, variant):
    _lib.call("bgnn_gemm_set_cfg", -1)
    _lib.call("bgnn_set_tuning", 5, 2)
    _lib.call("bgnn_gemm_set_cfg", cfg)
    _lib.call("bgnn_gemm_b16_variant", variant)


def up8(x):
    return (x + 7) // 8 * 8


def odd(x):
    return x + 1 if x % 2 == 0 else x + 2


def layout(c):
    """lda, ldb, ldc, ld0 (elements of the stored type) and the element shifts of A, B, C, bias, tables"""
    M, N, K, lay = c["M"], c["N"], c["K"], c["lay"]
    wa, wb = (M if c["ta"] else K), (K if c["tb"] else N)
    L = dict(lda=wa, ldb=wb, ldc=N, ld0=N, sa=0, sb=0, sc=0, sbias=0, st=0)
    if lay == "vec":
        L.update(lda=up8(wa) + 8, ldb=up8(wb) + 8, ldc=up8(N) + 8, ld0=up8(N) + 8)
    elif lay == "guard":
        L.update(lda=odd(wa), ldb=odd(wb), ldc=odd(N), ld0=odd(N), sa=1, sb=1, sc=1, sbias=1, st=1)
    elif lay:   # "<variant>-<the route it takes>"
        named = {"lda+8": dict(lda=wa + 8), "ldb+16": dict(ldb=wb + 16), "ldc+8": dict(ldc=N + 8), "ldc+4": dict(ldc=N + 4),
                 "ldc+1": dict(ldc=N + 1), "c-off": dict(sc=1), "bias-off4": dict(sbias=1), "ld0+4": dict(ld0=N + 4),
                 "ld0+1": dict(ld0=N + 1), "table-off4": dict(st=1)}
        L.update([v for k, v in named.items() if lay.startswith(k)][0])
    return L


class Ws:
    """a workspace of `nbytes` followed by a guard"""

    def __init__(self, dev, nbytes):
        self.nbytes = nbytes
        self.buf = torch.full((nbytes + 256,), WS_FILL, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr() if nbytes else None

    def guard(self, label):
        assert bool((self.buf[self.nbytes:] == WS_FILL).all()), f"{label}: bytes after the {self.nbytes}-byte workspace overwritten"


def run_gemm(dev, c, st, variant, ops):
    """one call of bgnn_gemm_bf16 / bgnn_gemm_gather_add_bf16 with storage st; the bf16 or f32 C on the host"""
    M, N, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    d, L = R.gemm_inputs(c), layout(c)
    label = f"{R.gid(c)} storage {st} variant {variant} {L}"

    def op(name, t, ld, bf, shift):   # operands are shared by the storages and variants of a case
        key = (name, bf)
        if key not in ops:
            ops[key] = Buf(dev, t, ld, BF if bf else F32, shift)
        return ops[key]
    A = op("a", d["a"], L["lda"], st & 1, L["sa"])
    B = op("b", d["b"], L["ldb"], st & 2, L["sb"])
    bias = op("bias", d["bias"].view(1, N), N, 0, L["sbias"]) if c["bias"] else None
    C = Win(dev, M, N, L["ldc"], BF if st & 4 else F32, L["sc"], init=d["c0"] if c["beta"] != 0.0 else None)
    nws = _lib.query("bgnn_gemm_ws_bytes_ex", M, N, K, ta, tb, 1) if c["ws"] else 0
    if c["ws"]:   # split-K really planned
        assert nws >= R.D_SHAPES["f4"][3] * M * N * 4, f"{label}: the planner no longer splits K"
    ws = Ws(dev, nws)
    select(c["cfg"], variant)
    if c["tables"]:
        t0 = op("t0", d["add0"], L["ld0"], 0, L["st"])
        t1 = op("t1", d["add1"], L["ld0"], 0, L["st"]) if c["tables"] > 1 else None
        if "i0" not in ops:
            ops["i0"], ops["i1"] = d["idx0"].to(dev), (d["idx1"].to(dev) if t1 else None)
        _lib.call("bgnn_gemm_gather_add_bf16", M, N, K, A.ptr, L["lda"], B.ptr, L["ldb"], C.ptr, L["ldc"], ptr(bias),
                  c["relu"], t0.ptr, ops["i0"].data_ptr(), L["ld0"], ptr(t1), ptr(ops["i1"]), L["ld0"], st, ws.ptr,
                  ws.nbytes, _stream())
    else:
        _lib.call("bgnn_gemm_bf16", ta, tb, M, N, K, c["alpha"], A.ptr, L["lda"], B.ptr, L["ldb"], c["beta"], C.ptr,
                  L["ldc"], ptr(bias), c["relu"], st, ws.ptr, ws.nbytes, _stream())
    torch.cuda.synchronize()
    out = C.read()
    C.guard(label)
    ws.guard(label)
    return out, label


def check_gemm(c, st, out, label):
    d = R.gemm_inputs(c)
    sec = f"4d {c['sec']} {'bf16' if st & 4 else 'f32'} C"
    if c["data"] == "round":    # C == bf16(A) widened, bit for bit (a zero is +0)
        want = R.rounding_want(d["a"])
        fin = torch.isfinite(out.float())
        assert bool(fin.all()), f"{label}: {int((~fin).sum())} elements not finite"
        bad = (out.float().view(torch.int32) != want.view(torch.int32)).nonzero()
        assert bad.numel() == 0, (f"{label}: {bad.size(0)} elements differ from bf16(A); first at {bad[0].tolist()}: A "
                                  f"{d['a'][tuple(bad[0])].item()!r} ({d['a'].view(torch.int32)[tuple(bad[0])].item():#010x}), "
                                  f"got {out.float()[tuple(bad[0])].item()!r}, want {want[tuple(bad[0])].item()!r}")
        return
    ref, mag = R.gemm_ref(d["a"], d["b"], c["ta"], c["tb"], **R.gemm_kw(c, d))
    check(sec, out.float(), ref, R.c_bound(ref, mag, bool(st & 4)), label)
    if c["exact"]:
        want = R.round_c(ref) if st & 4 else ref.float()
        bad = (out.float() != want).nonzero()
        assert bad.numel() == 0, (f"{label}: exact data, {bad.size(0)} elements differ from the fp64 reference; first at "
                                  f"{bad[0].tolist()}: got {out.float()[tuple(bad[0])].item()!r}, want "
                                  f"{want[tuple(bad[0])].item()!r} (fp64 {ref[tuple(bad[0])].item()!r})")


@pytest.mark.parametrize("c", R.GEMM_CASES, ids=[R.gid(c) for c in R.GEMM_CASES])
def test_gemm(dev, c):
    """A, B, D: every storage of the case against the reference; C(storage | 4) == C(storage & 3).to(bfloat16)
    bit for bit; where both kernels take the case (A, B), the LDS-DMA kernel == the register-staged one"""
    ops, outs = {}, {}
    for st in c["sts"]:
        out, label = run_gemm(dev, c, st, c["variant"], ops)
        check_gemm(c, st, out, label)
        outs[st] = out
        if c["sec"] in ("A", "B") and c["variant"] == 0:
            x6, label6 = run_gemm(dev, c, st, -1, ops)
            assert torch.equal(x6.view(torch.int16 if st & 4 else torch.int32), out.view(torch.int16 if st & 4 else torch.int32)), \
                f"{label}: bgnn_gemm_b16_variant(0) and (-1) differ in bits"
    for st in c["sts"]:
        if st & 4 and st & 3 in outs:
            w = outs[st & 3].bfloat16()
            if c["data"] == "round":
                w = torch.where(w == 0, torch.zeros((), dtype=BF), w)
            assert torch.equal(outs[st].view(torch.int16), w.view(torch.int16)), \
                f"{R.gid(c)}: C(storage {st}) != C(storage {st & 3}).to(bfloat16)"


# ---------------------------------------------------------------------------------------------
# C. drop-add


@pytest.mark.parametrize("c", R.C_CASES, ids=[R.did(c) for c in R.C_CASES])
def test_dropadd(dev, c):
    """N = 256 / 512 with K % 64 == 0: the fused arm (st & 8) of the whole-line walk; N = 264: the LDS-DMA
    kernel, then bgnn_add_dropped_bf16; K = 96: the register-staged kernel, then bgnn_add_dropped_bf16.
    Against the reference on exact data, never against another kernel; A = 0: the zero pattern is the
    kept set."""
    M, N, K, p, seed = c["M"], c["N"], c["K"], c["p"], c["seed"]
    a, b, src = R.dropadd_inputs(M, N, K, c["data"])
    ref, bound, exact, keep = R.dropadd_ref(a, b, src, p, seed)
    label = R.did(c)
    A, B, S = Buf(dev, a, K, BF), Buf(dev, b, K, BF), Buf(dev, src, N, BF)
    C = Win(dev, M, N, N, BF)
    select(-1, 0)
    _lib.call("bgnn_gemm_bf16_dropadd", M, N, K, A.ptr, K, B.ptr, K, C.ptr, N, S.ptr, N, p, seed, _stream())
    torch.cuda.synchronize()
    out = C.read()
    C.guard(label)
    check("4d C drop-add", out.float(), ref, bound, label)
    first = R.r16((R.r16(a).to(D) @ R.r16(b).to(D).t()).float())
    assert torch.equal(out.float()[~keep], first[~keep]), f"{label}: a dropped element is not the rounded product"
    if exact:
        assert torch.equal(out, R.r16(ref.float()).bfloat16()), f"{label}: exact data, the bits differ from the reference"
    if c["data"]:
        assert torch.equal(out.float() != 0, keep), f"{label}: the kept set differs from the header's mask"


# ---------------------------------------------------------------------------------------------
# E. csrc/elem.hip


def _b16_window(dev, t):
    """a bf16 tensor as the window of a guarded allocation (an in-place operand)"""
    w = OutB16(dev, t.numel())
    w.buf[w.GUARD:w.GUARD + t.numel()] = t.view(torch.int16).to(dev)
    return w


@pytest.mark.parametrize("k,n,p,seed,flag", R.ELEM_CASES,
                         ids=[f"{e[0]}-{e[1]}-p{e[2]}-s{e[3] % 1000}-{e[4]}" for e in R.ELEM_CASES])
def test_elementwise(dev, k, n, p, seed, flag):
    """n = 8: one thread; 2040: not a multiple of the block; 8 * 256 * 8192 + 8: one element group past the
    grid cap of 8192 blocks, so the grid-stride loop runs. add_dropout: b NULL (flag 0) or given;
    add_dropped: a separate output (flag 0) or in place on a."""
    a, b = R.elem_inputs(n)
    label = f"E {k} n={n} p={p} seed={seed} flag={flag}"
    bd = Buf(dev, b.view(-1, 8), 8, BF)
    if k == "dropout":
        ad, out = Buf(dev, a.view(-1, 8), 8, BF), OutB16(dev, n)
        _lib.call("bgnn_add_dropout_bf16", ad.ptr, bd.ptr if flag else None, n, p, seed, out.ptr, _stream())
        torch.cuda.synchronize()
        got = out.read()
        out.guard(label)
        want, keep = R.add_dropout_ref(a, b if flag else None, p, seed)
        fin = torch.isfinite(got.float())
        assert bool(fin.all()), f"{label}: {int((~fin).sum())} elements not finite"
        nz = (a.float() + (b.float() if flag else 0)) != 0
        assert torch.equal((got != 0)[nz], keep[nz]), f"{label}: the kept set differs from the header's mask"
        bad = (got.view(torch.int16) != want.view(torch.int16)) & ~((got == 0) & (want == 0))
        assert not bool(bad.any()), f"{label}: {int(bad.sum())} elements differ from round16((a + b) * ik)"
        RATIOS["4d E add_dropout (mismatches)"] = max(RATIOS.get("4d E add_dropout (mismatches)", 0.0), float(bad.sum()))
        return
    aw = _b16_window(dev, a)
    out = aw if flag else OutB16(dev, n)
    _lib.call("bgnn_add_dropped_bf16", aw.ptr, bd.ptr, n, p, seed, out.ptr, _stream())
    torch.cuda.synchronize()
    got = out.read()
    out.guard(label)
    aw.guard(label + " (a)")
    if not flag:
        assert torch.equal(aw.read().view(torch.int16), a.view(torch.int16)), f"{label}: a was modified"
    ref, bound, keep = R.add_dropped_ref(a, b, p, seed)
    check("4d E add_dropped", got.float().view(1, -1), ref.view(1, -1), bound.view(1, -1), label)
    untouched = ~keep | (b == 0)
    assert torch.equal(got[untouched].view(torch.int16), a[untouched].view(torch.int16)), \
        f"{label}: a dropped (or zero) b element changed a"
    nzb = b != 0   # (a kept non-zero b moves a by more than half an ulp of a: |b ik| >= 1/8, |a| < 8)
    assert torch.equal((got.float() != a.float())[nzb], keep[nzb]), f"{label}: the kept set differs from the header's mask"
    if p == 0:
        assert torch.equal(got, (a.float() + b.float()).bfloat16()), f"{label}: p = 0 is not exact"


@pytest.mark.parametrize("Rr,H,mean,exact", R.SEG_CASES, ids=[f"R{c[0]}-H{c[1]}-mean{c[2]}-exact{c[3]}" for c in R.SEG_CASES])
def test_segments(dev, Rr, H, mean, exact):
    """degrees 0, 1, 7, 8, 9, 16, 17, 700 (the 8-in-flight loop and its tail), the last row empty; R = 3:
    fewer rows than one block's waves; R = 32772: past the 4 * 8192 rows of the capped grid; ldx / ldo padded."""
    rowptr, col, E = R.seg_csr(Rr)
    x, g = R.seg_inputs(Rr, H, exact)
    label = f"E segments R={Rr} H={H} mean={mean} exact={exact}"
    rp, cl = rowptr.to(dev), col.to(dev)
    X = Buf(dev, x, H + 8, BF)
    out = Win(dev, Rr, H, H + 4, F32)
    _lib.call("bgnn_segment_sum_bf16", rp.data_ptr(), cl.data_ptr(), Rr, X.ptr, H + 8, H, mean, out.ptr, H + 4, _stream())
    torch.cuda.synchronize()
    got = out.read()
    out.guard(label + " sum")
    ref, bound = R.segment_sum_ref(rowptr, col, x, mean, bool(exact))
    check(f"4d E segment_{'mean' if mean else 'sum'}{'' if exact else ' random'}", got, ref, bound, label)
    if exact and not mean:
        assert torch.equal(got.to(D), ref), f"{label}: an integer sum is not exact"
    G = Buf(dev, g, H + 4, F32)
    o16 = Win(dev, E, H, H + 8, BF)
    _lib.call("bgnn_segment_bcast_bf16", rp.data_ptr(), cl.data_ptr(), Rr, G.ptr, H + 4, H, mean, o16.ptr, H + 8, _stream())
    torch.cuda.synchronize()
    got16 = o16.read()
    o16.guard(label + " bcast")
    want = R.segment_bcast_ref(rowptr, col, g, mean)
    assert bool(torch.isfinite(got16.float()).all()), f"{label}: bcast left positions unwritten"
    assert torch.equal(got16.view(torch.int16), want.view(torch.int16)), \
        f"{label}: bcast differs from (g / cnt).to(bfloat16) at {int((got16.view(torch.int16) != want.view(torch.int16)).sum())} elements"
