"""Host references for the LDS-resident VALU kernels at the two ends of every model and the BatchNorm
of the per-module path: csrc/mlp.hip (bgnn_mlp2_fwd / _bwd, bgnn_small_linear_fwd / _bwd,
bgnn_linear_bwd_prep_bf16), csrc/head.hip (bgnn_head2_fwd / _bwd) and csrc/bn.hip (bgnn_bn_stats /
_apply / _bwd_stats / _bwd_dx). fp64 evaluations of the formulas in include/bgnn.h on the same f32
(or bf16) inputs; each returns (ref, bound) or a dict of them. No GPU is touched here.

Bounds follow from the operation counts under the standard f32 model (u = 2^-24); none is measured:
  - a dot product of n fma terms plus a bias: (n + 1) u (sum |terms| + |bias|), in any order;
  - a value computed from a rounded intermediate carries the intermediate's bound through in fp64
    as sum |coefficient| bound(intermediate) (ReLU is 1-Lipschitz), and the magnitudes of its own
    roundings take |intermediate| + bound(intermediate);
  - a sum over rows follows the structure the code fixes: a workgroup (slot) adds at most R rows,
    the two-stage slot sum at most ceil(slots / 16) + 16 more, so (R + ceil(slots / 16) + 16 + 3) u
    sum |terms| + u |result| (tree_bound of sage_rows_ref), with R from the documented partition.

ReLU masks carry no exclusions: where a kernel recomputes a hidden layer and masks on it, the
backward cases draw x, W1, b1 on a dyadic grid (x a multiple of 2^-4 in [-4, 4], W1 of 2^-5 in
[-1, 1], b1 of 2^-9 in [-1, 1]): every pre-activation and every partial sum of it is a multiple of
2^-9 below 2^10 in size, at most 19 bits, exact in f32 in any order with or without fma, so the
kernel's mask is the reference's; some pre-activations are exactly 0 (a zero x row with b1[k] = 0)
under non-zero upstream gradients. Where the mask comes from an input array, that array is made on
the host, independent of x: about half exact zeros (among them -0.0), the rest positive normals.

Mutations: every reference takes `mut`, one deliberate mistake of MUTATIONS; tests/
test_dense_rows_ref.py shows that each leaves the true result by more than 8 x the bound."""
import functools

import torch

from sage_rows_ref import D, U, _cycle, _prod, _seed, colsum, tree_bound

KT = 64                     # csrc/mlp.hip: constexpr int kT = 64 (nodes per tile)
MLP_BLOCKS = 256            # csrc/mlp.hip: constexpr int kMlpBlocks = 256 (the backward's grid, one slot each)
MLP_FWD_BLOCKS = 2 * 256    # csrc/mlp.hip, bgnn_mlp2_fwd: mlp_blocks(N, 2 * kMlpBlocks)
SUM_GROUPS = 16             # csrc/mlp.hip: kSumGroups; csrc/head.hip: kHeadSumGroups
BN_BLOCKS = 1024            # csrc/bn.hip: constexpr int kBnBlocks = 1024
BN_ROWS_BLOCKS = 8192       # csrc/bn.hip, rows_blocks: if (b > 8192) b = 8192 (blocks of 256 float4)
PREP_BLOCKS = 512           # csrc/mlp.hip: constexpr int kPrepBlocks = 512
MLP_F, MLP_D1, MLP_D2 = 16, 64, 128   # csrc/mlp.hip: kF, kD1, kD2
HEAD_D1 = 64                # csrc/head.hip: kHD1

MUTATIONS = ("drop_last_row", "drop_second_tile_row", "skip_last_slot", "skip_group_slot", "mask_ge_h", "mask_ge_h1",
             "mask_ge_y", "no_b1", "no_b2", "no_bias", "w2_last_row", "cg4_col", "unshifted_var", "n_minus_1",
             "sums_swapped", "lane_tail", "amax_not_accumulated")


def zero():
    return torch.zeros((), dtype=D)


# ============================================================================ the tile partition
def tile_partition(N, T, cap):
    """(slots, R): a persistent grid of min(tiles, cap) workgroups (at least 1) walks the tiles of T
    rows with a stride of the grid; workgroup b owns slot b and adds at most R = T ceil(tiles / slots)
    rows into it."""
    tiles = -(-N // T)
    slots = min(max(tiles, 1), cap)
    return slots, T * -(-tiles // slots)


def sum_depth(slots, R):
    """additions behind one summed element: R rows in the slot, ceil(slots / 16) slots per group, 16 groups"""
    return R + -(-slots // SUM_GROUPS) + SUM_GROUPS


def row_keep(N, T, cap, mut):
    """fp64 [N] of ones, with the rows a row-sum mutation leaves out set to 0"""
    keep = torch.ones(N, dtype=D)
    slots, _ = tile_partition(N, T, cap)
    slot = (torch.arange(N) // T) % slots
    if mut == "drop_last_row":
        keep[N - 1] = 0
    elif mut == "drop_second_tile_row":
        assert N > slots * T + 1, "no workgroup has a second tile"
        keep[slots * T + 1] = 0
    elif mut == "skip_last_slot":
        keep[slot == slots - 1] = 0
    elif mut == "skip_group_slot":   # the first slot of the last non-empty sum group
        per = -(-slots // SUM_GROUPS)
        keep[slot == (slots - 1) // per * per] = 0
    return keep


# ============================================================================ two dense layers
def _bias(b, n, off):
    return torch.zeros(n, dtype=D) if b is None or off else b.to(D)


def two_layer_fwd_ref(x, W1, b1, W2, b2, relu_out, mut=None):
    """y = [ReLU](ReLU(x W1^T + b1) W2^T + b2): (ref, bound).
    Layer 1 is a dot of D0 terms plus a bias: e1 = (D0 + 1) u (|x| |W1|^T + |b1|). Layer 2 carries e1
    through |W2| and adds its own (D1 + 1) u ((h1 + e1) |W2|^T + |b2|); both ReLUs are 1-Lipschitz."""
    xd, W1d, W2d = x.to(D), W1.to(D), W2.to(D).clone()
    b1d, b2d = _bias(b1, W1.size(0), mut == "no_b1"), _bias(b2, W2.size(0), mut == "no_b2")
    if mut == "w2_last_row":
        W2d[-1] = 0
    pre = xd @ W1d.t() + b1d
    e1 = (W1.size(1) + 1) * U * (xd.abs() @ W1d.abs().t() + b1d.abs())
    h1 = pre.clamp_min(0)
    y = h1 @ W2d.t() + b2d
    bound = e1 @ W2d.abs().t() + (W2.size(1) + 1) * U * ((h1 + e1) @ W2d.abs().t() + b2d.abs())
    return (y.clamp_min(0) if relu_out else y), bound


def is_dyadic_hidden(x, W1, b1):
    """the inputs lie on the grid that makes every pre-activation exact in f32"""
    def grid(t, step, lim):
        t = t.to(D) * step
        return bool((t == t.round()).all()) and bool((t.abs() <= lim * step).all())
    return grid(x, 16, 4) and grid(W1, 32, 1) and (b1 is None or grid(b1, 512, 1)) and W1.size(1) <= 128


def two_layer_bwd_ref(x, W1, b1, W2, g2, T, cap, mut=None, want_dx=False):
    """The backward of both layers given g2 = dL/d(layer-2 pre-activation) (exact: an input, or an
    input masked by an input), on a dyadic hidden layer (h1 exact, see the module text):
      dW2 = g2^T h1, db2 = sum g2: row sums of exact factors;
      g1 = (g2 W2) (.) [h1 > 0]: a dot of C = rows(W2) terms, e1 = (C + 1) u |g2| |W2| where the mask
         passes, exactly 0 (bound 0) elsewhere;
      dW1 = g1^T x, db1 = sum g1: row sums of terms that carry e1: sum e1 |x| on top of the row-sum
         bound, whose magnitudes take |g1| + e1;
      dx = g1 W1: a dot of D1 terms: e1 |W1| + (D1 + 1) u (|g1| + e1) |W1|.
    Returns a dict name -> (ref, bound)."""
    assert is_dyadic_hidden(x, W1, b1), "the backward references need the dyadic hidden layer"
    N = x.size(0)
    xd, W1d, W2d, W2m, gd = x.to(D), W1.to(D), W2.to(D), W2.to(D).clone(), g2.to(D)
    if mut == "w2_last_row":
        W2m[-1] = 0
    pre = xd @ W1d.t() + _bias(b1, W1.size(0), mut == "no_b1")
    mask = pre >= 0 if mut == "mask_ge_h1" else pre > 0
    h1 = pre.clamp_min(0)
    keep = row_keep(N, T, cap, mut).unsqueeze(1)
    slots, R = tile_partition(N, T, cap)
    depth = sum_depth(slots, R)
    out = {}
    dW2, db2 = (gd * keep).t() @ h1, (gd * keep).sum(0)
    if mut == "cg4_col":
        dW2[4:], db2[4:] = 0, 0
    out["dW2"] = (dW2, tree_bound(depth, gd.abs().t() @ h1, dW2))
    out["db2"] = (db2, tree_bound(depth, gd.abs().sum(0), db2))
    g1 = torch.where(mask, gd @ W2m, zero())
    e1 = torch.where(mask, (W2.size(0) + 1) * U * (gd.abs() @ W2d.abs()), zero())
    m1 = g1.abs() + e1
    dW1, db1 = (g1 * keep).t() @ xd, (g1 * keep).sum(0)
    out["dW1"] = (dW1, e1.t() @ xd.abs() + tree_bound(depth, m1.t() @ xd.abs(), dW1))
    out["db1"] = (db1, e1.sum(0) + tree_bound(depth, m1.sum(0), db1))
    if want_dx:
        out["dx"] = (g1 @ W1d, e1 @ W1d.abs() + (W1.size(0) + 1) * U * (m1 @ W1d.abs()))
    return out


def mlp2_fwd_ref(x, W1, b1, W2, b2, mut=None):
    return two_layer_fwd_ref(x, W1, b1, W2, b2, True, mut)


def mlp2_bwd_ref(x, W1, b1, W2, h, dh, mut=None):
    """g2 = dh (.) [h > 0] on the given h (exact), then the two layers; slots and R from kT = 64 and
    the grid of 256"""
    g2 = torch.where(h >= 0 if mut == "mask_ge_h" else h > 0, dh, torch.zeros((), dtype=dh.dtype))
    return two_layer_bwd_ref(x, W1, b1, W2, g2, KT, MLP_BLOCKS, mut)


def head2_fwd_ref(x, W1, b1, W2, b2, mut=None):
    return two_layer_fwd_ref(x, W1, b1, W2, b2, False, mut)


def head2_bwd_ref(x, W1, b1, W2, dy, tile, grid, mut=None):
    """tile, grid: bgnn_head2_geometry(0), (2)"""
    return two_layer_bwd_ref(x, W1, b1, W2, dy, tile, grid, mut, want_dx=True)


def amax_ref(prev, out, mut=None):
    """*amax after the call: max(previous value, max |out|) (f32 values, exact)"""
    m = float(out.abs().max()) if out.numel() else 0.0
    return m if mut == "amax_not_accumulated" else max(float(torch.tensor(prev, dtype=torch.float32)), m)


# ============================================================================ small_linear
def small_linear_fwd_ref(x, W, bias, relu, mut=None):
    """y = act(x W^T + bias): a dot of K terms (64 lanes of K / 256 terms, a shuffle tree of 6) plus a
    bias: (K + 1) u (|x| |W|^T + |bias|). mut 'lane_tail': the float4 groups past the last full 64."""
    K = x.size(1)
    xd, Wd = x.to(D), W.to(D)
    bd = _bias(bias, W.size(0), mut == "no_bias")
    bound = (K + 1) * U * (xd.abs() @ Wd.abs().t() + bd.abs())
    if mut == "lane_tail":
        full = (K // 4) // 64 * 64 * 4
        xd = xd[:, :full]
        Wd = Wd[:, :full]
    y = xd @ Wd.t() + bd
    return (y.clamp_min(0) if relu else y), bound


def small_linear_bwd_ref(gy, y, x, W, mut=None):
    """g = gy (.) [y > 0] (y given; exact); dW = g^T x and db = sum g: one thread adds the B rows in
    order, (B + 1) u sum |terms|; dx = g W: a dot of N terms, (N + 1) u |g| |W|."""
    B, N = gy.shape
    g = gy.to(D)
    if y is not None:
        g = torch.where(y >= 0 if mut == "mask_ge_y" else y > 0, g, zero())
    gk = g.clone()
    if mut == "drop_last_row" and B:
        gk[B - 1] = 0
    xd, Wd = x.to(D), W.to(D)
    return dict(dW=(gk.t() @ xd, (B + 1) * U * (g.abs().t() @ xd.abs())),
                db=(gk.sum(0), (B + 1) * U * g.abs().sum(0)),
                dx=(g @ Wd, (N + 1) * U * (g.abs() @ Wd.abs())))


# ============================================================================ linear_bwd_prep_bf16
def prep_bf16_rows_per_slot(n, C):
    """a block takes rpi = 256 / (C / 8) rows per step, the grid of 512 blocks strides over the rows:
    a slot adds at most rpi ceil(n / (512 rpi)) rows"""
    rpi = 256 // (C // 8)
    return rpi * -(-n // (PREP_BLOCKS * rpi))


def prep_bf16_ref(g, y, mut=None):
    """(g_out bf16, bit-exact: a mask on the bits; fp64 column sums of g_out; their bound)"""
    n, C = g.shape
    go = g if y is None else torch.where(y >= 0 if mut == "mask_ge_y" else y > 0, g, torch.zeros((), dtype=g.dtype))
    s, bound = colsum(go.float(), prep_bf16_rows_per_slot(n, C), mut="skip_row" if mut == "drop_last_row" else None)
    return go, s, bound


# ============================================================================ BatchNorm1d
def bn_slots(n, C):
    """(slots, rows per slot, rpi) of csrc/bn.hip's bn_blocks: ceil(n / rpi) blocks, rpi = 256 / (C / 4),
    at most 1024 and at least 1; a block takes ceil(n / blocks) consecutive rows"""
    rpi = 256 // (C // 4)
    blocks = min(max(-(-n // rpi), 1), BN_BLOCKS)
    return blocks, -(-n // blocks), rpi


def _bn_rows(t, n, C, mut):
    """rows a column-sum mutation leaves out"""
    if mut == "skip_last_slot":
        blocks, rpb, _ = bn_slots(n, C)
        return t[:(-(-n // rpb) - 1) * rpb]
    return t


def bn_stats_ref(x, mut=None):
    """shifted sums with k = x's first row: sum (x - k), sum (x - k)^2. A slot adds at most rpb rows;
    the difference and the square are the + 3 of colsum. Returns ((s0, bound), (s1, bound))."""
    n, C = x.shape
    R = bn_slots(n, C)[1]
    xd = x.to(D)
    d = xd - xd[0]
    cm = "skip_row" if mut == "drop_last_row" else None
    a = colsum(_bn_rows(d, n, C, mut), R, mut=cm)
    b = colsum(_bn_rows(xd * xd if mut == "unshifted_var" else d * d, n, C, mut), R, mut=cm)
    return a, b


def bn_bwd_stats_ref(g, x, mean, invstd, mut=None):
    """sum g, sum g xhat, xhat = (x - mean) invstd (difference and two products: the + 3)"""
    n, C = x.shape
    R = bn_slots(n, C)[1]
    gd = g.to(D)
    t = gd * ((x.to(D) - mean.to(D)) * invstd.to(D))
    cm = "skip_row" if mut == "drop_last_row" else None
    return colsum(_bn_rows(gd, n, C, mut), R, mut=cm), colsum(_bn_rows(t, n, C, mut), R, mut=cm)


def bn_apply_ref(x, scale, shift):
    """y = x scale + shift: the product and the sum (or one fma): 2 u (|x scale| + |shift|)"""
    t = x.to(D) * scale.to(D)
    return t + shift.to(D), 2 * U * (t.abs() + shift.to(D).abs())


def bn_bwd_dx_ref(g, x, mean, invstd, gamma, sums, mut=None):
    """dx = kA g - kB - xhat kC, kA = gamma invstd, kB = kA sums[0] / N, kC = kA sums[1] / N: kA one
    rounding, kB and kC three more (1 / N, two products), xhat two, the three products and the two
    differences: at most 10 u (|kA g| + |kB| + |xhat kC|), the count of bwd_rows_ref for this formula."""
    n = x.size(0)
    s = sums.to(D)
    if mut == "sums_swapped":
        s = s.flip(0)
    nn = n - 1 if mut == "n_minus_1" else n
    kA = (gamma.to(D) if gamma is not None else 1.0) * invstd.to(D)
    kB, kC = kA * s[0] / nn, kA * s[1] / nn
    t1, t3 = kA * g.to(D), (x.to(D) - mean.to(D)) * invstd.to(D) * kC
    return t1 - kB - t3, 10 * U * (t1.abs() + kB.abs() + t3.abs())


# ============================================================================ inputs
def dyadic(shape, step, lim, q):
    """multiples of 1 / step in [-lim, lim]"""
    k = int(lim * step)
    return torch.randint(-k, k + 1, shape, generator=q).float() / step


def mask_array(shape, q):
    """a host-made ReLU output: about half exact zeros (every other one of them -0.0), the rest positive
    normal numbers in [0.5, 1.5)"""
    v = torch.rand(shape, generator=q) + 0.5
    z = torch.rand(shape, generator=q) < 0.5
    v[z] = 0.0
    flat = v.view(-1)
    idx = z.view(-1).nonzero().flatten()[::2]
    flat[idx] = -0.0
    return v


BOOST = 256.0   # the upstream gradient of the rows a mutation singles out (a power of two)


@functools.lru_cache(maxsize=8)
def two_layer_inputs(N, D0, D1, D2, grid, T=KT, cap=MLP_BLOCKS, tag=0):
    """x [N, D0], W1 [D1, D0], b1, W2 [D2, D1], b2, the upstream gradient g [N, D2] and (for the encoder)
    a host-made h [N, D2]. grid: the dyadic hidden layer, with zero x rows (1 and N / 2, for N >= 4) and
    b1 = 0 at hidden units 0, 5, D1 - 1: exact-zero pre-activations. The rows the mutations single out
    (the zero rows, the last row, row 1 of a workgroup's second tile) carry BOOST x the gradient."""
    q = torch.Generator().manual_seed(_seed(N, D0, D1, D2, grid, tag, 41))
    if grid:
        x, W1, b1 = dyadic((N, D0), 16, 4, q), dyadic((D1, D0), 32, 1, q), dyadic((D1,), 512, 1, q)
        zr = sorted({1, N // 2}) if N >= 4 else []
        x[zr] = 0
        b1[[0, 5, D1 - 1]] = 0
    else:
        x, W1, b1 = torch.randn(N, D0, generator=q), torch.randn(D1, D0, generator=q) * D0 ** -0.5, \
            torch.randn(D1, generator=q) * 0.1
        zr = []
    W2, b2 = torch.randn(D2, D1, generator=q) * D1 ** -0.5, torch.randn(D2, generator=q) * 0.1
    g = torch.randn(N, D2, generator=q)
    slots, _ = tile_partition(N, T, cap)
    boost = set(zr) | {N - 1} | ({slots * T + 1} if N > slots * T + 1 else set())
    g[sorted(boost)] *= BOOST
    h = mask_array((N, D2), q)
    return dict(x=x, W1=W1, b1=b1, W2=W2, b2=b2, g=g, h=h, zero_rows=zr)


@functools.lru_cache(maxsize=8)
def small_linear_inputs(B, K, N):
    q = torch.Generator().manual_seed(_seed(B, K, N, 43))
    x, W, bias = torch.randn(B, K, generator=q), torch.randn(N, K, generator=q) * K ** -0.5, torch.randn(N, generator=q)
    gy, y = torch.randn(B, N, generator=q), mask_array((B, N), q)
    if B:
        gy[B - 1] = torch.where(gy[B - 1] < 0, -BOOST, BOOST)    # the last row shows in every column sum ...
        if B > 1:
            y[B - 1] = 1.0                                       # ... and passes the mask
    return dict(x=x, W=W, bias=bias, gy=gy, y=y)


@functools.lru_cache(maxsize=8)
def prep_bf16_inputs(n, C):
    """bf16 g, y: y host-made (half zeros, -0.0 among them); the last row passes the mask with |g| = 256"""
    q = torch.Generator().manual_seed(_seed(n, C, 47))
    g, y = torch.randn(n, C, generator=q), mask_array((n, C), q)
    if n > 1:
        y[n - 1] = 1.0
    g[n - 1] = torch.where(g[n - 1] < 0, -BOOST, BOOST)
    return g.bfloat16(), y.bfloat16()


@functools.lru_cache(maxsize=4)
def bn_inputs(n, C, kind):
    """x (kind 0: randn * 0.3 + 0.05; 1: 1e3 + randn), g, the f32 mean / invstd of x (biased variance,
    eps = 1e-5), gamma, scale / shift, and sums [2, C] (the f32 column sums of g and g xhat)"""
    q = torch.Generator().manual_seed(_seed(n, C, kind, 53))
    x = torch.randn(n, C, generator=q) * 0.3 + 0.05 if kind == 0 else 1e3 + torch.randn(n, C, generator=q)
    g = torch.randn(n, C, generator=q)
    if n:
        g[n - 1] = torch.where(g[n - 1] < 0, -BOOST, BOOST)
        x[n - 1] += 64.0 if n > 1 else 0.0                    # (an outlier: it shows in the sums of x - k)
    xd = x.to(D)
    mean = xd.mean(0) if n else torch.zeros(C, dtype=D)
    var = xd.var(0, unbiased=False) if n else torch.ones(C, dtype=D)
    invstd = 1.0 / (var + 1e-5).sqrt()
    gamma = torch.rand(C, generator=q) + 0.5
    beta = torch.randn(C, generator=q)
    mean32, is32 = mean.float(), invstd.float()
    xhat = (xd - mean32.to(D)) * is32.to(D)
    sums = torch.stack([g.to(D).sum(0), (g.to(D) * xhat).sum(0)]).float()
    scale = (gamma.to(D) * invstd).float()
    shift = (beta.to(D) - mean * gamma.to(D) * invstd).float()
    return dict(x=x, g=g, mean=mean32, invstd=is32, gamma=gamma, scale=scale, shift=shift, sums=sums)


# ============================================================================ the matrix
# A: N, (NULL biases: 0 none, 1 b1, 2 b2, 3 both; W2 4 bytes off a 16-byte boundary; amax: 0 NULL, 1 previous 0,
#    2 previous 3e30; dyadic inputs)
MLP_FWD_NS = (1, 63, 64, 65, 64 * 512 + 65)
MLP_FWD_CASES = [(n, (i % 4, (i // 2) % 2, i % 3, (i // 3) % 2))
                 for i, n in enumerate(n for n in MLP_FWD_NS for _ in range(4))]
# B: N, b1 NULL
MLP_BWD_NS = (1, 63, 65, 64 * 17, 64 * 256 + 65)
MLP_BWD_CASES = [(n, nb) for n in MLP_BWD_NS for nb in (0, 1)]
# C: (B, K, N), forward (relu, bias NULL) / backward (y NULL, db NULL, dx NULL)
SL_SHAPES = _prod((1, 3, 200), (4, 64, 252, 256, 260, 1024), (1, 3, 64, 65))[::5]
SL_FWD_CASES = _cycle(SL_SHAPES, _prod((1, 0), (0, 1)), 2)
SL_BWD_CASES = _cycle(SL_SHAPES, _prod((0, 1), (0, 1), (0, 1))[::3] + [(1, 1, 1)], 2)
# D: (D0, C), N index (the last N from the geometry), (b1 NULL, b2 NULL)
HEAD_SHAPES = _prod((64, 128), (1, 2, 4, 5, 7, 8))
HEAD_CASES = [((d0, c), (2 * i + j) % 6, ((i + j) % 2, (i // 2 + j) % 2))
              for i, (d0, c) in enumerate(HEAD_SHAPES) for j in range(2)]


def head_ns(tile, grid):
    return (1, tile - 1, tile, tile + 1, tile * 17, tile * grid + tile + 1)


# E: (N, C), y given
PREP16_CASES = [((n, c), f) for n in (1, 5, 257, 5000) for c in (8, 16, 256, 2048) for f in (1, 0)]
# F: (C, n_rows), input kind, gamma NULL
BN_CS = (4, 8, 64, 512, 1024)


def bn_rows_list(C):
    rpi = 256 // (C // 4)
    return sorted({n for n in (1, 2, rpi - 1, rpi, rpi + 1, BN_BLOCKS * rpi + 1) if n > 0})


BN_CASES = [((C, n), (i + j) % 2, (i + j // 2) % 2) for i, C in enumerate(BN_CS) for j, n in enumerate(bn_rows_list(C))]
BN_STRIDE_CASE = (1024, 8193)    # more than 8192 * 256 float4: the grid-stride second pass of the row kernels


def case_id(c):
    def flat(v):
        return "-".join(flat(x) for x in v) if isinstance(v, (tuple, list)) else str(v)
    return flat(c)
