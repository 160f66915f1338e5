"""Host references for the bf16 gather skeleton (csrc/b16_gather.h) and the entry points instantiated
from it -- bgnn_spmm_fwd_bf16, bgnn_spmm_bwd_bf16, bgnn_spmm_max_bf16, bgnn_spmm_max_pack_bf16,
bgnn_sage_infer_bf16, bgnn_sage_fwd_bf16 -- and for bgnn_sage_tail_bf16, which shares sage_tail.h's
tail: the case lists, the inputs (bf16 rows, exact in f32 and in fp64), fp64 evaluations of the
formulas of include/bgnn.h on the upcast rows, the bounds that follow from their operation counts
(u = 2^-24; nothing here is a measured tolerance), the combine and key-batch geometry restated from
the documented rules, and the mutations shared by tests/test_gpu_agg_b16_matrix.py (GPU) and
tests/test_agg_b16_ref.py (CPU: agreement with independent statements, teeth). No GPU is touched.

Structure. The kinds are tests/spmm_ref.py's, plus `dense` (spmm_ref.dense_edges: groups of 64, 65,
256 and 512 keys) as planned with 4 and with 8 rows per group. A heavy row's chunks go to the 16
waves of combine_chunks in runs of per = ceil(chunks / 16): hand_c4 holds rows of 16, 17 and 175
chunks (per 1, 2 with waves 9..15 idle, 11), hand_c16 one of 44 (per 3, 15 runs).

Inputs. Every bf16 value is exact in f32, so the f32 references of spmm_ref / sage_rows_ref apply
to the upcast rows unchanged. Rows of the gathered plane (x, g, z_l) that no edge of the direction
names hold NaN: the references never read them (they index by edge), a kernel that gathers a wrong
row does.

Bounds.
  sums (A)   spmm_ref.fwd_ref / bwd_ref's: (cnt - 1 + k) u sum |terms|, k = 0 (SUM), 2 (MEAN: the
             correctly rounded reciprocal and one product per element or per term). On the exact
             input (integers in [-3, 3], every partial sum an integer below 2^24) the bound is 0.
  max (B)    exact.
  layer (C)  o = h / max(||h||, 1e-12) carries sage_rows_ref.sage_fwd_ref's o_bound (h: (cnt + 4) u mag;
             the norm: first order in dh plus (H + 8) u nrm; the quotient 2 u |o|). The tail computes
             t = fl(fma(o, scale, shift)), v = max(t, 0), y = fl(v + x_prev): the error of o passes
             through the product as |scale| o_bound, ReLU is 1-Lipschitz, and the two roundings add at
             most u |o scale + shift| + u (|v| + |x_prev|) <= 2 u (|o scale| + |shift|) + u |x_prev|.
             The bound takes sage_apply_ref's 5 u (|o scale| + |shift| + |x_prev|) (its p = 0 case):
               |scale| o_bound + 5 u (|o scale| + |shift| + |x_prev|).
             Without scale / shift nothing is computed before the ReLU: o_bound, plus 2 u (|v| +
             |x_prev|) for the one rounding of the skip addition. The tail alone is the same formula
             with a zero aggregate (cnt = 0: h = y + b).
  layer (D)  o and nrm: sage_fwd_ref's o_bound and nrm_bound. BatchNorm slots, against the STORED o:
             a slot adds R rows' values in some order, so the fp64 sum over the slots is within
             (Rmax - 1) u sum |o| of the fp64 column sum of o, and within Rmax u sum o^2 for the
             squares (one more rounding each); Rmax = sage_rows_ref.fwd_rows_per_slot. A heavy row's
             slot is its o bit for bit, and its square plane within u o^2.

Mutations: every reference takes `mut`, one deliberate mistake of MUTATIONS (or of spmm_ref's), and
computes what a subtly wrong kernel would; tests/test_agg_b16_ref.py shows each leaves the true
result by more than 8 x the bound on the matrix's own inputs."""
import functools

import torch

import sage_rows_ref as SR
import spmm_ref as R
from sage_rows_ref import D, U, away, ratio   # noqa: F401  (shared with the GPU matrix)

SUM, MEAN = R.SUM, R.MEAN
BF = torch.bfloat16
NAN = float("nan")
W_COMBINE = 16          # kCombineWaves (csrc/seg_common.h)
KEY_BATCH = 64          # keys per batch of walk_groups

MUTATIONS = ("combine_floor", "idle_wave_garbage", "batch2_lost", "mask_tail_absorbed", "last_lane_bias",
             "norm_drops_lane", "zr_from_zl", "mean_scales_zr", "relu_then_affine", "skip_inside_relu",
             "h_rounded_bf16", "slot_of_wrong_row")
STRUCTURAL = MUTATIONS[:4]

# ============================================================================ the cases
KINDS = R.HAND + ("hand_t", "store") + R.CHUNKED + R.TINY + ("dense", "dense_r8")
H_FULL = (8, 24, 64, 72, 200, 256, 264, 504, 512)
H_SHORT = (8, 200, 504, 512)
CASES = [("hand", h) for h in H_FULL] + [(k, h) for k in KINDS[1:] for h in H_SHORT]
IDS = [f"{k}-{h}" for k, h in CASES]

# rows per group of the plan each kind runs on (0: no plan, one row per wave; store: explicit starts)
GROUP_ROWS = {"hand_r8": 8, "dense_r8": 8, "hand_nogroups": 0, "hand_c200": 0}
# the gather batch of the row-group kernels (k_*_group<4, 8> and <8, 4>)
GATHER_U = {4: 8, 8: 4}


def group_rows(kind):
    return GROUP_ROWS.get(kind, 4)


# bgnn_sage_fwd_bf16_slots per kind, written out by hand from the documented rule: grid8(n_groups,
# 1024) for a row-group plan of 4 or 8 rows with chunk <= 64, else grid8(n_rows, 2048) -- grid8(w, cap)
# = min(ceil(w / 4), cap) rounded up to a multiple of 8, at least 8 -- plus one per heavy row.
#   (light-row blocks, heavy rows)
EXPECT_SLOTS = {
    "hand": (64, 2),             # 251 groups of 4 -> 63 blocks -> 64; rows 11 and 500
    "hand_r8": (32, 2),          # 126 groups of 8 -> 32
    "hand_nogroups": (256, 2),   # 1,003 rows -> 251 blocks -> 256
    "hand_t": (64, 0),           # the reversed hand graph's forward rows are the hand graph's sources: <= 64 entries
    "hand_c4": (64, 419),        # every row above 4 entries
    "hand_c16": (64, 3),         # rows 10, 11 and 500
    "hand_c200": (256, 1),       # chunk 200 > 64: no row-group plan; row 500
    "tiny1": (8, 0), "tiny3": (8, 0), "tiny5": (8, 1), "tiny9": (8, 0),
    "dense": (40, 1),            # 150 groups of 4 -> 38 -> 40; row 40
    "dense_r8": (24, 1),         # 75 groups of 8 -> 19 -> 24
    "store": (64, 3),            # 246 groups (explicit starts, per graph) -> 62 -> 64; the super nodes
}


def grid8(w, cap):
    return max(8, (min(-(-w // 4), cap) + 7) // 8 * 8)


def expect_slots(kind, n_groups=None):
    """(light-row blocks, heavy rows, (group_rows, n_groups) or None) of a kind's forward CSR"""
    S = R.struct(kind)
    light, heavy = EXPECT_SLOTS[kind]
    nh = int((S.deg > S.chunk).sum())
    assert heavy is None or heavy == nh, f"{kind}: {nh} heavy rows, {heavy} written out"
    rows = group_rows(kind)
    grouped = rows in (4, 8) and S.chunk <= 64
    if grouped and n_groups is None:
        n_groups = -(-S.n // rows)
    rule = grid8(n_groups, 1024) if grouped else grid8(S.n, 2048)
    assert light is None or light == rule, f"{kind}: the rule gives {rule} light-row blocks, {light} written out"
    return rule, nh, ((rows, n_groups) if grouped else None)


# ============================================================================ structure restated
def chunks_of(kind, transposed=False):
    """{heavy row: its chunk count}"""
    S = R.struct(kind)
    deg = S.deg_t if transposed else S.deg
    return {int(r): -(-int(deg[r]) // S.chunk) for r in (deg > S.chunk).nonzero().flatten()}


def combine_runs(chunks):
    """(per, non-empty runs) of combine_chunks for a row of `chunks` chunks"""
    per = -(-chunks // W_COMBINE)
    return per, -(-chunks // per)


@functools.lru_cache(maxsize=None)
def edge_keys(kind, rows, transposed=False):
    """bgnn_group_plan restated for groups of `rows` consecutive rows (grow = NULL): per column of
    edge_index the key index of that entry within its group (-1: a heavy row's entry, which the plan
    leaves out), and gcnt per group. A group's keys are (source, occurrence of that source earlier in
    the same row), numbered by first appearance over its light rows' entries in row order."""
    S = R.struct(kind)
    rowptr, col, order, deg = (S.rowptr_t, S.col_t, S.order_t, S.deg_t) if transposed else (S.rowptr, S.col, S.order, S.deg)
    key = torch.full((S.E,), -1, dtype=torch.int64)
    gcnt = []
    colv, ordv, rp = col.tolist(), order.tolist(), rowptr.tolist()
    for r0 in range(0, S.n, rows):
        keys = {}
        for r in range(r0, min(r0 + rows, S.n)):
            if int(deg[r]) > S.chunk:
                continue
            seen = {}
            for p in range(rp[r], rp[r + 1]):
                k = (colv[p], seen.get(colv[p], 0))
                seen[colv[p]] = k[1] + 1
                key[ordv[p]] = keys.setdefault(k, len(keys))
        gcnt.append(len(keys))
    return key, torch.tensor(gcnt, dtype=torch.int64)


def edge_weights(kind, transposed, mut):
    """How often a mutated kernel adds each entry (fp64 over the columns of edge_index; 1 everywhere
    for a correct one), for the slips of b16_gather.h:
      combine_floor       per = floor(chunks / 16): a row of more than 16 chunks loses the chunks
                          from 16 floor(chunks / 16) on
      idle_wave_garbage   a wave whose run is empty adds the chunk its clamped start names (the
                          row's last) once more
      batch2_lost         a group's keys from the 65th on are dropped (the eb > 0 reload)
      mask_tail_absorbed  the masked slots of a group's last gather batch add the batch's first key
                          once more to the rows that hold it
    -> (weights, whether any differs from 1)"""
    S = R.struct(kind)
    deg, off, tgt = (S.deg_t, S.off_t, S.ei[0]) if transposed else (S.deg, S.off, S.ei[1])
    w = torch.ones(S.E, dtype=D)
    ch, nch = off // S.chunk, -(-deg[tgt] // S.chunk)
    heavy = deg[tgt] > S.chunk
    if mut == "combine_floor":
        w[heavy & (nch > W_COMBINE) & (ch >= W_COMBINE * (nch // W_COMBINE))] = 0
    elif mut == "idle_wave_garbage":
        per = -(-nch // W_COMBINE)
        idle = W_COMBINE - -(-nch // per.clamp_min(1))
        last = heavy & (ch == nch - 1)
        w[last] += idle[last].to(D)
    elif mut in ("batch2_lost", "mask_tail_absorbed"):
        rows = group_rows(kind)
        if rows in (4, 8) and S.chunk <= 64 and kind != "store":   # (store: the group starts are the batch's)
            key, gcnt = edge_keys(kind, rows, transposed)
            if mut == "batch2_lost":
                w[key >= KEY_BATCH] = 0
            else:
                u = GATHER_U[rows]
                cnt = gcnt[tgt // rows]
                first = cnt - cnt % u                   # the first key of the last, partly masked batch
                hit = (key >= 0) & (cnt % u != 0) & (key == first)
                w[hit] += (u - cnt % u)[hit].to(D)
    else:
        raise ValueError(mut)
    return w, bool((w != 1).any())


# ============================================================================ inputs
def unnamed(kind, transposed=False):
    """bool [N]: the rows of the gathered plane that no edge of the direction names (forward: never a
    source; transpose: never a target)"""
    S = R.struct(kind)
    named = torch.zeros(S.n, dtype=torch.bool)
    named[S.ei[1] if transposed else S.ei[0]] = True
    return ~named


def poisoned(kind, x, transposed=False):
    x = x.clone()
    x[unnamed(kind, transposed)] = NAN
    return x


@functools.lru_cache(maxsize=None)
def randn_b16(kind, H, salt=0, transposed=False):
    """bf16 [N, H] standard normal (spmm_ref.randn_rows rounded), NaN in the unnamed rows"""
    return poisoned(kind, R.randn_rows(kind, H, salt).to(BF), transposed)


@functools.lru_cache(maxsize=None)
def exact_b16(kind, H, transposed=False):
    """integers in [-3, 3]: every partial sum of at most 2^22 of them is an integer below 2^24"""
    n = R.edges(kind)[1]
    g = torch.Generator().manual_seed(R._seed(kind, H, 41 + int(transposed)))
    return poisoned(kind, torch.randint(-3, 4, (n, H), generator=g).to(BF), transposed)


@functools.lru_cache(maxsize=None)
def subbf16_rows(kind, H):
    """f32 [N, H] for the pack kernel: values of a four-element bf16 set times 1 + k 2^-12, k in 0..7
    varying with row and column: below bf16 precision (half an ulp is 2^-9 relative at least), so rows
    that tie after rounding have a strict f32 winner, which is often not the first edge"""
    n = R.edges(kind)[1]
    g = torch.Generator().manual_seed(R._seed(kind, H, 43))
    base = torch.tensor([0.0, 1.0, 1.5, -2.0])[torch.randint(0, 4, (n, H), generator=g)]
    k = torch.randint(0, 8, (n, H), generator=g).float()
    x = base * (1 + k * 2.0 ** -12)
    assert torch.equal(x.to(BF).float(), base)
    return x


def max_input(kind, H, which):
    """the f32 rows of a MAX case (the bf16 kernel takes them rounded: ties, infinities and NaN survive)"""
    return {"randn": lambda: R.randn_rows(kind, H, 0), "ties": lambda: R.ties_rows(kind, H),
            "nonfinite": lambda: R.nonfinite_rows(kind, H), "subbf16": lambda: subbf16_rows(kind, H)}[which]()


def zero_row(kind):
    """the first isolated row (it gets z_r = 0: with no bias h = 0), or None"""
    iso = (R.struct(kind).deg == 0).nonzero().flatten()
    return int(iso[0]) if iso.numel() else None


@functools.lru_cache(maxsize=None)
def layer_inputs(kind, H):
    """dict(z bf16 [N, 2H] with NaN in the z_l plane of the unnamed rows and z_r = 0 in zero_row,
    bias f32 [H], scale, shift f32 [H], xprev bf16 [N, H])"""
    n = R.edges(kind)[1]
    g = torch.Generator().manual_seed(R._seed(kind, H, 47))
    z = torch.randn(n, 2 * H, generator=g).to(BF)
    z[:, :H] = poisoned(kind, z[:, :H])
    zr = zero_row(kind)
    if zr is not None:
        z[zr, H:] = 0
    return dict(z=z, bias=0.5 * torch.randn(H, generator=g), scale=torch.rand(H, generator=g) + 0.5,
                shift=0.1 * torch.randn(H, generator=g), xprev=torch.randn(n, H, generator=g).to(BF))


@functools.lru_cache(maxsize=None)
def tail_inputs(n, H):
    g = torch.Generator().manual_seed(SR._seed(n, H, 53))
    y = torch.randn(n, H, generator=g).to(BF)
    y[n // 2] = 0                                  # with no bias: a zero-norm row
    return dict(y=y, bias=0.5 * torch.randn(H, generator=g), scale=torch.rand(H, generator=g) + 0.5,
                shift=0.1 * torch.randn(H, generator=g), xprev=torch.randn(n, H, generator=g).to(BF))


# ============================================================================ A. sums
def sum_ref(kind, xb, reduce, transposed=False, mut=None):
    """bgnn_spmm_fwd_bf16 / bgnn_spmm_bwd_bf16 on the upcast rows: spmm_ref.fwd_ref / bwd_ref and their
    bound (mut: one of spmm_ref's, or a structural one of this module) -> (fp64 result, bound)"""
    x = xb.float()
    if mut is None or mut in R.MUTATIONS:
        return R.bwd_ref(kind, x, reduce, None, mut) if transposed else R.fwd_ref(kind, x, reduce, mut)
    S = R.struct(kind)
    w = edge_weights(kind, transposed, mut)[0].view(-1, 1)
    src, dst = S.ei[0], S.ei[1]
    out = torch.zeros(S.n, x.size(1), dtype=D)
    if transposed:
        s = 1.0 / S.deg[dst].clamp_min(1).to(D).view(-1, 1) if reduce == MEAN else 1.0
        out.index_add_(0, src, w * s * x.to(D)[dst])
    else:
        out.index_add_(0, dst, w * x.to(D)[src])
        if reduce == MEAN:
            out = out / S.deg.clamp_min(1).to(D).view(-1, 1)
    return out, None


# ============================================================================ C / D. the layer
def _flags(bias, d):
    return d["bias"] if bias else None


def layer_ref(kind, z, bias, mean, mut=None):
    """h = s sum z_l[col] + z_r + b, nrm = ||h||, o = h / max(nrm, 1e-12) on the upcast bf16 z.
    mut None: sage_rows_ref.sage_fwd_ref (o, o_bound, nrm, nrm_bound, h). Otherwise this module's own
    fp64 evaluation with one slip: a structural one (edge_weights), or
      last_lane_bias   no bias on the last 8 columns        norm_drops_lane  the norm omits them
      zr_from_zl       z_r read at column 0 of z            mean_scales_zr   s (a + z_r)
      h_rounded_bf16   h rounded to bf16 before the norm
    mut 'own': the same evaluation without a slip (the CPU test compares it with sage_fwd_ref)."""
    S = R.struct(kind)
    H = z.size(1) // 2
    b = bias if bias is not None else torch.zeros(H)
    if mut is None:
        return SR.sage_fwd_ref(S.ei, S.n, z[:, :H].float(), z[:, H:].float(), b, mean)
    zd, b = z.to(D), b.to(D).clone()
    w = edge_weights(kind, False, mut)[0] if mut in STRUCTURAL else torch.ones(S.E, dtype=D)
    agg = torch.zeros(S.n, H, dtype=D).index_add_(0, S.ei[1], w.view(-1, 1) * zd[:, :H][S.ei[0]])
    s = (1.0 / S.deg.clamp_min(1).to(D) if mean else torch.ones(S.n, dtype=D)).view(-1, 1)
    zr = zd[:, :H] if mut == "zr_from_zl" else zd[:, H:]
    if mut == "last_lane_bias":
        b[-8:] = 0
    h = s * (agg + zr) + b if mut == "mean_scales_zr" else s * agg + zr + b
    if mut == "h_rounded_bf16":
        h = h.float().to(BF).to(D)
    nrm = (h[:, :-8] if mut == "norm_drops_lane" else h).pow(2).sum(1).sqrt()
    return dict(h=h, nrm=nrm, o=h / nrm.clamp_min(1e-12).unsqueeze(1))


def apply_ref(o, o_bound, scale, shift, xprev, mut=None):
    """y = ReLU(o scale + shift) + x_prev in fp64 with the bound of the module docstring.
    mut 'relu_then_affine': ReLU(o) scale + shift; 'skip_inside_relu': ReLU(o scale + shift + x_prev)."""
    xp = xprev.to(D) if xprev is not None else None
    if scale is None:
        v = o.clamp_min(0)
        if mut == "skip_inside_relu" and xp is not None:
            return (o + xp).clamp_min(0), None
        y = v + xp if xp is not None else v
        return y, o_bound + (2 * U * (v + xp.abs()) if xp is not None else 0)
    sc, sh = scale.to(D), shift.to(D)
    t = o * sc
    if mut == "relu_then_affine":
        y = o.clamp_min(0) * sc + sh
    elif mut == "skip_inside_relu" and xp is not None:
        return (t + sh + xp).clamp_min(0), None
    else:
        y = (t + sh).clamp_min(0)
    if xp is not None:
        y = y + xp
    return y, sc.abs() * o_bound + 5 * U * (t.abs() + sh.abs() + (xp.abs() if xp is not None else 0))


def infer_ref(kind, d, mean, affine, skip, bias, mut=None):
    """bgnn_sage_infer_bf16 on layer_inputs d under the flags -> (fp64 y, bound)"""
    tail_mut = mut in ("relu_then_affine", "skip_inside_relu")
    true = layer_ref(kind, d["z"], _flags(bias, d), mean)
    L = true if mut is None or tail_mut else layer_ref(kind, d["z"], _flags(bias, d), mean, mut)
    return apply_ref(L["o"], true["o_bound"], d["scale"] if affine else None, d["shift"] if affine else None,
                     d["xprev"] if skip else None, mut if tail_mut else None)


def tail_ref(d, affine, skip, bias, mut=None):
    """bgnn_sage_tail_bf16: the same formula with a zero aggregate (no edges: cnt = 0, h = y + b)"""
    n, H = d["y"].shape
    b = d["bias"] if bias else torch.zeros(H)
    none = torch.zeros(2, 0, dtype=torch.int64)
    L = SR.sage_fwd_ref(none, n, torch.zeros(n, H), d["y"].float(), b, 0)
    return apply_ref(L["o"], L["o_bound"], d["scale"] if affine else None, d["shift"] if affine else None,
                     d["xprev"] if skip else None, mut)


def slot_sums_ref(o, rmax, heavy=(), mut=None):
    """the fp64 column sums of the stored o and o^2 with their bounds: (Rmax - 1) u sum |o| and
    Rmax u sum o^2. mut 'slot_of_wrong_row': every heavy row's slot holds its neighbour's o."""
    od = o.to(D).clone()
    if mut == "slot_of_wrong_row":
        for r in heavy:
            od[r] = o[r - 1 if r else r + 1].to(D)
    a = o.to(D)
    return (od.sum(0), (rmax - 1) * U * a.abs().sum(0)), ((od * od).sum(0), rmax * U * (a * a).sum(0))


# ============================================================================ the flag cycles
def _walk(flags, stride):
    """the flag product in an order that changes every flag often (a stride coprime to its length)"""
    return [flags[(stride * i) % len(flags)] for i in range(len(flags))]


# C: (kind, H), (mean, affine, skip, bias): four consecutive tuples of this walk hold both values of
# every flag, so every case meets every flag value
INFER_CASES = SR._cycle(CASES, _walk(SR._prod((0, 1), (1, 0), (0, 1), (1, 0)), 7), 4)
# C, the tail alone: (N, H), (affine, skip, bias)
TAIL_CASES = SR._cycle(SR._prod(SR.NS, H_SHORT), _walk(SR._prod((1, 0), (0, 1), (1, 0)), 3), 4)
# D: (kind, H), (mean, bias): the full product
FWD_CASES = [(c, f) for c in CASES for f in SR._prod((0, 1), (1, 0))]
