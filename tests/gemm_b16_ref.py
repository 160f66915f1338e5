"""Host references for the bf16-STORAGE GEMM family (bgnn_gemm_bf16, bgnn_gemm_gather_add_bf16,
bgnn_gemm_bf16_dropadd: csrc/gemm_b16.hip, csrc/gemm_x6_b16s.hip) and the bf16 helpers of
csrc/elem.hip (bgnn_add_dropout_bf16, bgnn_add_dropped_bf16, bgnn_segment_sum_bf16,
bgnn_segment_bcast_bf16): fp64 evaluations of the formulas of include/bgnn.h on the same inputs
(each with `mag`, the fp64 sum of the absolute values of the terms behind an element), the bounds,
the inputs and the case lists shared by tests/test_gpu_gemm_b16_matrix.py (GPU) and
tests/test_gemm_b16_ref.py (CPU: agreement with plain torch, an f32 host evaluation, mutations).
No GPU is touched here.

Bounds (none is measured on the code under test).
  f32 C, random data   REL * mag + TINY, the per-element class of tests/test_gpu_gemm_matrix.py
  bf16 C, random data  2^-8 |ref| + (1 + 2^-8) x the f32 bound: one nearest rounding to 8 significant bits
  exact data           operands integers in [-3, 3], bias / gathered rows / C0 multiples of 1/8 (C0: of 1/2,
                       times beta = 1/4) below 8, K <= 512: every partial sum in any order is a multiple of
                       2^-3 below 2^11, 14 bits, so the f32 C EQUALS the fp64 reference and the bf16 C EQUALS
                       its nearest-even rounding (assert_exact_data checks the premise on the reference)
  rounding set         B = I: C is bf16(A) widened, bit for bit. The sum runs from a +0 accumulator, so
                       a zero result is +0 whatever the sign of the zero (or underflowed) operand: IEEE
                       addition, (+0) + (-0) = +0
  add_dropout_bf16     round16((a + b) * ik): two f32 operations restated in numpy float32 (no fused
                       multiply-add is possible across them), one rounding: exact
  add_dropped_bf16     a + w ik may or may not be contracted: 2^-8 |exact| + 2 u (|a| + |w ik|); dropped
                       and zero b leave a exactly, p = 0 (and ik a power of two on exact data) is exact
  drop-add GEMM        round16(round16(A B^T) + drop(src)): the same bound around the exactly rounded
                       product of exact data; exact for p = 0 and p = 0.5
  segment_sum_bf16     (cnt - 1) u sum |terms| (any order), + 2 u sum |terms| for mean (the correctly
                       rounded reciprocal and its product)
  segment_bcast_bf16   equals torch's (g / cnt).to(bfloat16) per position

Mutations: every reference takes `mut`, one deliberate mistake of MUTATIONS, and computes what a
subtly wrong kernel would; tests/test_gemm_b16_ref.py shows that each leaves the true result by more
than 8 bounds, or changes a bit of an exact case, at every case meant to show it (SHOWS)."""
import functools

import numpy as np
import torch

from sage_rows_ref import D, SEEDS, U, _cycle, _prod, away, dropout_threshold, inv_keep, keep_mask, ratio  # noqa: F401

REL = 2e-6              # tests/test_gpu_gemm_matrix.py's per-element class (REL, TINY there)
TINY = 1e-37
E16 = 2.0 ** -8         # half an ulp of bf16 (8 significant bits), relative
# (bm, bn) of the bf16-operand tiles 0..4 (kX6Cfgs in csrc/gemm_x6.hip; X6_TILES[:5] of the GEMM matrix)
TILES = [(128, 128), (256, 128), (128, 256), (256, 256), (256, 256)]
D_SHAPES = {"f4": (150, 132, 1041, 4)}   # tests/test_gpu_gemm_matrix.py's split-K shape used here

MUTATIONS = ("drop_last_k64", "clamp_row", "idx_prev", "idx_swap", "bias_256", "relu_early", "trunc_operand",
             "trunc_c", "no_first_round", "group_shift", "no_ik", "deg_plus_1", "no_clamp", "drop_ninth")


def shape_of(variant, bm, bn):
    """tests/test_gpu_gemm_matrix.py's shape_of"""
    return {"unal": (bm + 37, bn + 22, 79), "al": (bm + 40, bn + 36, 96)}[variant]


def r16(x, trunc=False):
    """f32 -> the nearest-even bf16 value (torch CPU), as f32; trunc: the low 16 bits cut instead"""
    x = x.float().contiguous()
    if trunc:
        return (x.view(torch.int32) & -65536).view(torch.float32)
    return x.bfloat16().float()


def gen(*key):
    s = 23
    for k in key:
        s = (s * 1000003 + int(k)) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(s)


def ints(g, *shape, lo=-3, hi=3):
    return torch.randint(lo, hi + 1, shape, generator=g).float()


def eighths(g, *shape):
    """multiples of 1/8 with |v| < 8"""
    return torch.randint(-63, 64, shape, generator=g).float() / 8


# ============================================================================ the GEMM
def gemm_ref(a, b, ta, tb, alpha=1.0, beta=0.0, c0=None, bias=None, relu=False, add0=None, idx0=None, add1=None,
             idx1=None, mut=None):
    """fp64 act(alpha op(A) op(B) + beta C0 + bias + add0[idx0] + add1[idx1]) of the bf16-rounded
    operands, and mag = the sum of |terms|. a / b as stored: [M, K] or [K, M] (ta), [K, N] or [N, K] (tb)."""
    t = mut == "trunc_operand"
    A, B = r16(a, t).to(D), r16(b, t).to(D)
    A = A.t() if ta else A
    B = B.t() if tb else B
    M, K = A.shape
    N = B.size(1)
    if mut == "drop_last_k64" and K > 0:
        k0 = (K - 1) // 64 * 64
        A = A[:, :k0]
        B = B[:k0]
    if mut == "clamp_row" and M > 1:
        A = A.clone()
        A[M - 1] = A[M - 2]
    ref, mag = alpha * (A @ B), abs(alpha) * (A.abs() @ B.abs())
    if beta != 0.0:
        ref, mag = ref + beta * c0.to(D), mag + abs(beta) * c0.to(D).abs()
    if bias is not None:
        bv = bias.to(D).clone()
        if mut == "bias_256":
            bv[256:264] = 0
        ref, mag = ref + bv, mag + bv.abs()
    if mut == "relu_early" and relu:
        ref = ref.clamp_min(0)
    if add0 is not None:
        i0 = idx0.clone()
        i1 = None if idx1 is None else idx1.clone()
        if mut == "idx_prev" and M > 1:
            i0[M - 1] = i0[M - 2]
            if i1 is not None:
                i1[M - 1] = i1[M - 2]
        if mut == "idx_swap" and i1 is not None:
            i0 = i1
        g0 = add0.to(D).index_select(0, i0)
        ref, mag = ref + g0, mag + g0.abs()
        if add1 is not None:
            g1 = add1.to(D).index_select(0, i1)
            ref, mag = ref + g1, mag + g1.abs()
    if relu and mut != "relu_early":
        ref = ref.clamp_min(0)
    return ref, mag


def c_bound(ref, mag, c16):
    f32 = REL * mag + TINY
    return E16 * ref.abs() + (1 + E16) * f32 if c16 else f32


def round_c(ref, mut=None):
    """the bf16 C of an exact case: the nearest-even rounding of the (f32-exact) reference"""
    assert torch.equal(ref.float().to(D), ref)
    return r16(ref.float(), mut == "trunc_c")


def assert_exact_data(ref):
    """the premise of the exact cases: no bit below 2^-3, |ref| < 2^11"""
    assert bool((ref * 8 == (ref * 8).round()).all()) and float(ref.abs().max() if ref.numel() else 0.0) < 2 ** 11


def host_f32(a, b, ta, tb, alpha=1.0, beta=0.0, c0=None, bias=None, relu=False, add0=None, idx0=None, add1=None,
             idx1=None, reverse=False):
    """an f32 host evaluation in the kernels' order: the 64-deep k slices summed in natural or reversed
    order, then alpha, beta C0, bias, the gathered rows, ReLU"""
    A, B = r16(a), r16(b)
    A = A.t() if ta else A
    B = B.t() if tb else B
    M, K = A.shape
    acc = torch.zeros(M, B.size(1))
    ks = list(range(0, K, 64))
    for k0 in (reversed(ks) if reverse else ks):
        acc = acc + A[:, k0:k0 + 64].contiguous() @ B[k0:k0 + 64].contiguous()
    v = acc * np.float32(alpha)
    if beta != 0.0:
        v = v + np.float32(beta) * c0
    if bias is not None:
        v = v + bias
    if add0 is not None:
        v = v + add0[idx0]
        if add1 is not None:
            v = v + add1[idx1]
    return v.clamp_min(0) if relu else v


# ---------------------------------------------------------------------------- cases and inputs
def G(sec, M, N, K, ta=0, tb=1, sts=(3, 7), alpha=1.0, beta=0.0, bias=0, relu=0, exact=1, tables=0, rows=5, cfg=-1,
      variant=0, lay="", ws=0, data="", note=""):
    """One GEMM case: every storage of `sts` runs on it. lay: layout variants joined by '+' (run_gemm
    of the GPU matrix reads them); note: the branch the case is there for (it goes into the id)."""
    return dict(sec=sec, M=M, N=N, K=K, ta=ta, tb=tb, sts=tuple(sts), alpha=alpha, beta=beta, bias=bias, relu=relu,
                exact=exact, tables=tables, rows=rows, cfg=cfg, variant=variant, lay=lay, ws=ws, data=data, note=note)


def gid(c):
    s = f"{c['sec']}-{c['M']}x{c['N']}x{c['K']}-{'tn' if c['ta'] else 'nt'}-st{''.join(map(str, c['sts']))}"
    if c["cfg"] >= 0:
        s += f"-tile{c['cfg']}"
    s += f"-b{c['bias']}r{c['relu']}" + (f"-t{c['tables']}x{c['rows']}" if c["tables"] else "")
    if (c["alpha"], c["beta"]) != (1.0, 0.0):
        s += "-alphabeta"
    for k in ("lay", "data", "note"):
        if c[k]:
            s += "-" + c[k]
    return s + ("" if c["exact"] else "-random") + ("-x6" if c["variant"] else "") + ("-ws" if c["ws"] else "")


ROUND_BITS = (0x3F808000, 0x3F818000,                           # ties: even lower neighbour (down), odd (up)
              0x3F807FFF, 0x3F808001, 0x3F817FFF, 0x3F818001,   # one f32 ulp to either side of each
              0x3FFFFFFF, 0xBFFFFFFF,                           # the largest below a binade edge: up into the next
              0x00000000, 0x80000000,                           # +-0
              0x00000001, 0x00400000, 0x007FFFFF, 0x00008000, 0x00018000, 0x80018000,   # f32 subnormals (ties too)
              0x7F7F0000, 0xFF7F0000,                           # +-the largest finite bf16
              0xC2F6E979, 0x3DCCCCCD)                           # (ordinary values)


def rounding_a(M, K):
    """the rounding set: A [M, K] f32 with ROUND_BITS cycled over the columns, shifted by the row"""
    bits = np.array(ROUND_BITS, dtype=np.uint32)
    idx = (np.arange(K)[None, :] + np.arange(M)[:, None]) % len(bits)
    return torch.from_numpy(bits[idx].view(np.float32).copy())


def rounding_want(a):
    """bf16(A) widened; a zero (or a value that rounds to one) arrives as +0: (+0) + (-0) = +0"""
    w = r16(a)
    return torch.where(w == 0, torch.zeros(()), w)


@functools.lru_cache(maxsize=8)
def _gemm_inputs(key):
    c = dict(key)
    M, N, K, ta, tb = c["M"], c["N"], c["K"], c["ta"], c["tb"]
    g = gen(M, N, K, ta, tb, c["tables"], c["rows"], c["bias"], len(c["sec"]), ord(c["sec"][0]))
    d = dict(c0=None, bias=None, add0=None, idx0=None, add1=None, idx1=None)
    sa, sb = ((K, M) if ta else (M, K)), ((N, K) if tb else (K, N))
    if c["data"] == "round":
        assert (ta, tb) == (0, 1) and N == K
        d["a"], d["b"] = rounding_a(M, K), torch.eye(N)
    elif c["data"] == "zeroA":
        d["a"], d["b"] = torch.zeros(sa), ints(g, *sb)
    elif c["exact"]:
        d["a"], d["b"] = ints(g, *sa), ints(g, *sb)
    else:
        d["a"], d["b"] = torch.randn(sa, generator=g), torch.randn(sb, generator=g)
    # (stored-bf16 operands hold these values rounded by torch; the reference rounds every operand itself)
    draw = eighths if c["exact"] else (lambda q, *s: torch.randn(s, generator=q))
    if c["beta"] != 0.0:
        d["c0"] = (torch.randint(-15, 16, (M, N), generator=g).float() / 2) if c["exact"] else torch.randn(M, N, generator=g)
    if c["bias"]:
        d["bias"] = draw(g, N)
        if c["exact"] and N > 256:   # (bias_256 shows)
            d["bias"][256:264] = torch.where(d["bias"][256:264] == 0, torch.ones(()), d["bias"][256:264])
    if c["tables"]:
        R = c["rows"]
        d["add0"] = draw(g, R, N)
        # sorted with repeats; the last row alone takes the table's last row (idx_prev shows)
        i0 = torch.sort(torch.randint(0, R - 1, (M,), generator=g)).values
        i0[0], i0[-1] = 0, R - 1
        d["idx0"] = i0
        if c["tables"] > 1:
            d["add1"] = draw(g, R, N)
            i1 = torch.randint(0, R, (M,), generator=g)                      # random
            i1 = torch.where(i1 == i0, (i1 + 1) % R, i1)                     # (idx_swap shows)
            if M > 1:
                i1[-1] = [v for v in range(R) if v != int(i1[-2]) and v != int(i0[-1])][0]
            d["idx1"] = i1
    return d


def gemm_inputs(c):
    return _gemm_inputs(tuple(sorted((k, v) for k, v in c.items() if k not in ("sts", "cfg", "variant", "lay", "ws", "note"))))


def gemm_kw(c, d):
    return dict(alpha=c["alpha"], beta=c["beta"], c0=d["c0"], bias=d["bias"], relu=bool(c["relu"]), add0=d["add0"],
                idx0=d["idx0"], add1=d["add1"], idx1=d["idx1"])


BR = _prod((0, 1), (0, 1))   # (bias, ReLU): each on and off

# A. the LDS-DMA kernel, plain: wave tile 128 rows x 64 columns of a 256 x 256 workgroup tile.
#    N = 8 / 72: column blocks that end inside a wave's 64 columns -> the x6_epilogue fall-back (edge);
#    N = 256: every wave on the whole-line walk (bf16 C) / the 32-column block walk (f32 C, rows inside M);
#    N = 264 / 328: a second column tile holding 8 / 72 columns; M = 1 / 33 / 129: rows past M skipped row by
#    row (whole-line) or the fall-back (f32 C: the block walk needs all 128 rows), the glds row clamp;
#    M = 256 / 257: a full tile / one row in a second; K = 64 / 128 / 192: prologue only, one steady
#    iteration, the slot wrap of the two-slot pipeline.
A_SHAPES = _prod((1, 33, 129, 256, 257), (8, 72, 256, 264, 328), (64, 128, 192)) + [(520, 520, 64)]   # last: 9 tiles
A_CASES = [G("A", *s, bias=f[0], relu=f[1]) for s, f in _cycle(A_SHAPES, BR, 2)]
A_LAYOUTS = ("lda+8", "ldb+16", "ldc+8-fast", "ldc+4-x6-8B-stores", "ldc+1-x6-scalar-stores", "c-off-x6-scalar-stores",
             "bias-off4-x6")
A_CASES += [G("A", 257, 264, 128, bias=1, relu=1, lay=v) for v in A_LAYOUTS]
A_CASES += [G("A", 257, 264, 192, bias=1, relu=1, exact=0)]

# B. the LDS-DMA kernel, gathered: M = 257: the index copy's clamp at M - 1 (second row tile holds one
#    row); M = 129: wm = 1 holds one row; M = 300; the second table's LDS copy at li + BM.
B_SHAPES = _prod((1, 129, 257, 300), (72, 256, 328), (64, 192))
B_CASES = [G("B", *s, bias=f[0], relu=f[1], tables=f[2], rows=f[3])
           for s, f in _cycle(B_SHAPES, [(b, r, t, n) for (b, r) in BR for t in (1, 2) for n in (5, 997)][::3], 2)]
B_LAYOUTS = ("ld0+4-fast", "ld0+1-x6-global-idx", "table-off4-x6-global-idx")
B_CASES += [G("B", 257, 328, 64, bias=1, relu=1, tables=2, rows=997, lay=v) for v in B_LAYOUTS]
B_CASES += [G("B", 300, 328, 192, bias=1, relu=1, tables=2, rows=997, exact=0)]

# D. the register-staged storage kernels k_gemm_x6<2, ...>: every built (ta, tb, storage) on every forced tile
# (a storage with a bf16 C runs beside its f32-C form: C(storage | 4) == C(storage & 3).to(bfloat16) bit for bit)
D_COMBOS = [(0, 1, (1, 5)), (0, 1, (3, 7)), (0, 1, (0, 4)), (1, 0, (1,)), (1, 0, (2,)), (1, 0, (3,))]
# the layout goes with the shape: "al" shapes are "vec" = 16-byte aligned rows (the vector arms of x6_load<BF> / kq_load<BF> /
# kq_load16, 8-byte C16 stores), "unal" shapes are "guard" = every operand one element off a 16-byte boundary with an odd ld (the
# element-guarded arms), an odd ldc (scalar 2-byte C16 stores), C and the bias one element off; bias and ReLU
# are cycled over the product
D_CASES = []
for _i, ((_ta, _tb, _sts), _cfg, _v) in enumerate(_prod(D_COMBOS, range(5), ("unal", "al"))):
    _lay, (_b, _r) = ("guard" if _v == "unal" else "vec"), BR[(_i // 2 + _i // 10) % 4]
    D_CASES.append(G("D", *shape_of(_v, *TILES[_cfg]), ta=_ta, tb=_tb, sts=_sts, cfg=_cfg, bias=_b, relu=_r, lay=_lay))
# storage 3 / 7 NT at K % 64 == 0 kept off the LDS-DMA kernel by bgnn_gemm_b16_variant(-1)
D_CASES += [G("D", 257, 264, 128, bias=1, relu=1, variant=-1), G("D", 129, 72, 128, tables=2, rows=997, variant=-1)]
D_CASES += [G("D", 165, 150, 79, sts=(3,), alpha=0.5, beta=0.25, bias=1, relu=1, lay=v) for v in ("vec", "guard")]
# the TN storages with alpha, beta and a split-K workspace (K > 512: random data), and without one
D_CASES += [G("D", *D_SHAPES["f4"][:3], ta=1, tb=0, sts=(s,), alpha=0.75, beta=-0.5, bias=1, relu=1, exact=0, ws=w,
              lay="vec") for s in (1, 2, 3) for w in (1, 0)]
D_CASES += [G("D", 165, 150, 96, ta=1, tb=0, sts=(s,), alpha=0.5, beta=0.25, bias=1, lay="vec") for s in (1, 2, 3)]
D_CASES += [G("D", 70, 150, k, ta=ta, tb=1 - ta, sts=sts, bias=1, relu=r, lay="vec", note=f"K{k}")
            for k, r in ((0, 1), (8, 0)) for ta, sts in ((0, (1, 3, 4, 5, 7)), (1, (1, 2, 3)))]
D_CASES += [G("D", 165, 96, 96, sts=(0, 4), cfg=cfg, data="round", lay=lay, note="rounding-set")
            for cfg, lay in ((-1, "vec"), (0, "guard"), (1, "vec"), (2, "guard"), (3, "vec"), (4, "guard"))]

GEMM_CASES = A_CASES + B_CASES + D_CASES


# ============================================================================ the drop-add GEMM
def DA(M, N, K, p, seed, data=""):
    return dict(M=M, N=N, K=K, p=p, seed=seed, data=data)


def did(c):
    route = "fused-dropadd-arm" if c["N"] % 256 == 0 and c["K"] % 64 == 0 else \
        ("ldsdma+add_dropped" if c["K"] % 64 == 0 else "x6+add_dropped")
    return f"C-{c['M']}x{c['N']}x{c['K']}-p{c['p']}-s{c['seed'] % 1000}-{route}" + (f"-{c['data']}" if c["data"] else "")


C_CASES = [DA(M, N, K, p, SEEDS[i % 3]) for i, (p, M, N, K) in
           enumerate(_prod((0.0, 0.1, 0.5), (1, 255, 257), (256, 512, 264), (64, 192, 96)))]
C_CASES += [DA(257, N, 64, p, s, "zeroA-kept-set") for N in (256, 264) for p in (0.1, 0.5) for s in SEEDS]


@functools.lru_cache(maxsize=4)
def dropadd_inputs(M, N, K, data):
    g = gen(M, N, K, 77)
    # rows of one sign, B positive: |A B^T| ~ 4 K needs more than bf16's 8 bits (the first rounding rounds)
    a = torch.zeros(M, K) if data else ints(g, M, K, lo=1) * (1 - 2 * (torch.arange(M) % 2)).float().unsqueeze(1)
    src = ints(g, M, N, lo=-6, hi=6)
    src = torch.where(src == 0, torch.ones(()), src) if data else src     # (the zero pattern is the mask's alone)
    return a, ints(g, N, K, lo=1), src


def dropadd_ref(a, b, src, p, seed, mut=None):
    """round16(round16(A B^T) + drop(src)) before its last rounding: (fp64 value, bound, exact, keep).
    The mask group is (row * ld_src + col) / 4 with ld_src = N; kept values * f32(1 / (1 - p))."""
    M, N = a.size(0), b.size(0)
    prod = r16(a).to(D) @ r16(b).to(D).t()
    first = prod if mut == "no_first_round" else r16(prod.float()).to(D)
    keep = keep_mask(seed, M, N, p, "group_shift" if mut == "group_shift" else None)
    ik = 1.0 if mut == "no_ik" else float(inv_keep(p))
    w = torch.where(keep, src.to(D) * ik, torch.zeros((), dtype=D))
    ref = first + w
    exact = float(inv_keep(p)) in (1.0, 2.0)     # a power of two: the product and the sum are exact on integer data
    return ref, E16 * ref.abs() + 2 * U * (first.abs() + w.abs()), exact, keep


# ============================================================================ csrc/elem.hip
ELEM_N = (8, 2040, 8 * 256 * 8192 + 8)    # the last: one element group past the grid cap (8192 blocks of 256 x 8)
# (kernel, n, p, seed, flag): add_dropout with flag = b given; add_dropped with flag = in place on a. The small
# sizes take every (p, seed) pair of the mask; the large one is one pass per kernel.
ELEM_CASES = [(k, n, p, s, (i + j + f) % 2) for k in ("dropout", "dropped") for i, n in enumerate(ELEM_N[:2])
              for j, (p, s) in enumerate([(0.0, 0)] + _prod((0.1, 0.5), SEEDS)) for f in (0, 1)]
ELEM_CASES += [("dropout", ELEM_N[2], 0.1, SEEDS[2], 1), ("dropped", ELEM_N[2], 0.5, SEEDS[1], 1)]


@functools.lru_cache(maxsize=2)
def elem_inputs(n):
    """a, b bf16 [n]: eighths below 8 (their sum is exact in f32); b holds zeros"""
    g = gen(n, 5)
    a = eighths(g, n).bfloat16()
    b = eighths(g, n)
    b[::7] = 0
    return a, b.bfloat16()


def add_dropout_ref(a, b, p, seed, mut=None):
    """round16((a + b) * ik) on kept elements, 0 on dropped ones: bf16, exact"""
    n = a.numel()
    s = a.float().numpy() + (b.float().numpy() if b is not None else np.float32(0))     # f32 sum (exact here or not)
    keep = keep_mask(seed, 1, n, p, "group_shift" if mut == "group_shift" else None).view(-1).numpy()
    ik = np.float32(1.0) if mut == "no_ik" else inv_keep(p)
    v = np.where(keep, (s * ik).astype(np.float32), np.float32(0)) if dropout_threshold(p) else s
    return torch.from_numpy(np.ascontiguousarray(v, dtype=np.float32)).bfloat16(), torch.from_numpy(keep)


def add_dropped_ref(a, b, p, seed, mut=None):
    """a + drop(b): (fp64 value before the rounding, bound, keep)"""
    keep = keep_mask(seed, 1, a.numel(), p, "group_shift" if mut == "group_shift" else None).view(-1)
    ik = 1.0 if mut == "no_ik" else float(inv_keep(p))
    w = torch.where(keep, b.to(D) * ik, torch.zeros((), dtype=D))
    ref = a.to(D) + w
    return ref, E16 * ref.abs() + 2 * U * (a.to(D).abs() + w.abs()), keep


SEG_DEG = (0, 1, 7, 8, 9, 16, 17, 700, 3, 0)    # the 8-in-flight loop and its tail; the last row is empty
SEG_H = (8, 72, 512)
SEG_R = (len(SEG_DEG), 3, 32772)                # hand; fewer rows than one block's waves; past 4 * 8192 rows
SEG_CASES = [(R, H, mean, exact) for R in SEG_R for H in SEG_H for mean, exact in ((0, 1), (1, 1), (1, 0))
             if R != 32772 or H == 72]


@functools.lru_cache(maxsize=4)
def seg_csr(R):
    """(rowptr int32 [R + 1], col int32 [E], n_src): SEG_DEG (cycled for large R, without its 700) as a CSR
    whose col is a permutation of the positions"""
    deg = list(SEG_DEG) if R == len(SEG_DEG) else [1, 9, 0] if R == 3 else \
        [(0, 1, 7, 8, 9, 16, 17, 2, 3)[i % 9] for i in range(R - 1)] + [0]
    rowptr = torch.cat([torch.zeros(1, dtype=torch.int64), torch.cumsum(torch.tensor(deg), 0)])
    E = int(rowptr[-1])
    col = torch.randperm(E, generator=gen(R, 9)) if E else torch.zeros(0, dtype=torch.int64)
    return rowptr.to(torch.int32), col.to(torch.int32), E


@functools.lru_cache(maxsize=4)
def seg_inputs(R, H, exact):
    rowptr, col, E = seg_csr(R)
    g = gen(R, H, exact, 3)
    x = ints(g, E, H) if exact else torch.randn(E, H, generator=g)
    gr = torch.randn(R, H, generator=g)
    return x.bfloat16(), gr


def segment_sum_ref(rowptr, col, x, mean, exact=False, mut=None):
    """(fp64 sum or mean per row, bound). exact data (integers): the sum is exact in any order, its bound 0"""
    R, H = rowptr.numel() - 1, x.size(1)
    rp, cl = rowptr.long(), col.long()
    deg = rp[1:] - rp[:-1]
    seg = torch.repeat_interleave(torch.arange(R), deg)
    keep = torch.ones(cl.numel(), dtype=torch.bool)
    if mut == "drop_ninth":
        keep[(rp[:-1] + 8)[deg >= 9]] = False
    xs = x.to(D)[cl]
    s = torch.zeros(R, H, dtype=D).index_add_(0, seg[keep], xs[keep])
    mag = torch.zeros(R, H, dtype=D).index_add_(0, seg, xs.abs())
    cnt = deg.to(D).unsqueeze(1)
    bound = torch.zeros_like(mag) if exact else (cnt - 1).clamp_min(0) * U * mag
    if mean:
        den = cnt + 1 if mut == "deg_plus_1" else (cnt if mut == "no_clamp" else cnt.clamp_min(1))
        s, mag = s / den, mag / cnt.clamp_min(1)
        bound = bound / cnt.clamp_min(1) + 2 * U * mag
    return s, bound


def segment_bcast_ref(rowptr, col, g, mean):
    """bf16 [E, H]: position col[p] of segment r holds torch's (g[r] / max(deg, 1)).to(bfloat16)"""
    rp, cl = rowptr.long(), col.long()
    deg = rp[1:] - rp[:-1]
    v = (g / deg.clamp_min(1).float().unsqueeze(1)) if mean else g
    out = torch.zeros(cl.numel(), g.size(1), dtype=torch.bfloat16)
    out[cl] = v.bfloat16()[torch.repeat_interleave(torch.arange(deg.numel()), deg)]
    return out


# ============================================================================ which cases show which mutation
def shows(mut, c):
    """is GEMM case c meant to show GEMM mutation mut?"""
    if c["data"]:
        return mut == "trunc_operand" and c["data"] == "round" or mut == "trunc_c" and c["data"] == "round" and 4 in c["sts"]
    M, N, K = c["M"], c["N"], c["K"]
    return {"drop_last_k64": K > 0, "clamp_row": M > 1 and K > 0, "idx_prev": c["tables"] > 0 and M > 1,
            "idx_swap": c["tables"] > 1 and c["rows"] > 1, "bias_256": bool(c["bias"]) and N >= 264 and bool(c["exact"]),
            "relu_early": bool(c["relu"]) and c["tables"] > 0, "trunc_operand": not c["exact"],
            "trunc_c": any(s & 4 for s in c["sts"]) and K >= 64 and bool(c["bias"] or c["tables"]) and M * N >= 256 and bool(c["exact"])}.get(mut, False)
