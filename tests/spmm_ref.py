"""Host references for the f32 aggregation entry points of csrc/spmm.hip with the plain epilogue --
bgnn_spmm_fwd (SUM / MEAN / MAX and the argmax state), bgnn_spmm_bwd, bgnn_spmm_bwd_add,
bgnn_spmm_bwd_max -- and for the state bgnn_spmm_max_bf16 writes: the structure cases, the CSR order
(a stable sort on the host, never the device's), fp64 evaluations of the formulas of include/bgnn.h
on the same f32 inputs, the bounds that follow from their operation counts (u = 2^-24; nothing here
is a measured tolerance), the kernel geometry restated from the documented rules, the inputs and the
case lists shared by tests/test_gpu_spmm_matrix.py (GPU) and tests/test_spmm_ref.py (CPU: agreement
with the oracle, mutations). No GPU is touched here.

Bounds. A sum of cnt f32 terms in ANY order (the chunk and combine trees, the row-group key order,
the gather batches) is within (cnt - 1) u sum |terms| of the exact sum (Jeannerod & Rump 2013: no
higher-order term). k further roundings that touch every term add k u sum |terms|:
  SUM forward / transpose  k = 0   (the weight 1.f multiplies exactly)
  MEAN forward             k = 2   (inv_deg = fl(1 / deg), correctly rounded, and its product with the sum)
  MEAN transpose (MEANT)   k = 2   (w = fl(1 / deg_fwd(t)) and the product fl(g w) of every term)
  + addend                 the addend is one more term: cnt + 1 terms, cnt roundings, and sum |terms|
                           includes |addend|
  MAX backward             the sum bound over the matching edges (the others add an exact 0)
The MAX forward, amax and every bit-identity claim are exact.

Mutations: every reference takes `mut`, one deliberate mistake of MUTATIONS, and computes what a
subtly wrong kernel would; tests/test_spmm_ref.py shows each one leaves the true result by more than
8 x the bound."""
import functools

import torch

from sage_rows_ref import D, U, away, ratio   # noqa: F401  (shared with the GPU matrix)

NEG_INF = float("-inf")
SUM, MEAN, MAX = 0, 1, 2
MUTATIONS = ("drop_last", "drop_chunk", "deg_plus_1", "out_degree", "b64_heavy", "b65_light", "no_addend",
             "last_tie", "split_ties", "amax_no_prev")

# ============================================================================ structure cases
HAND = ("hand", "hand_r8", "hand_nogroups")
CHUNKED = ("hand_c4", "hand_c16", "hand_c200")
TINY = ("tiny1", "tiny3", "tiny5", "tiny9")
# in-degrees of the tiny graphs: fewer rows than XCDs (8) or than the 4 waves of a block; tiny3 and
# tiny9 end on an empty row; tiny5 holds a heavy row (70 > 64 edges drawn from 5 sources)
TINY_DEG = {0: [], 1: [3], 3: [3, 3, 0], 5: [2, 1, 4, 3, 70], 9: [1, 8, 2, 5, 3, 4, 6, 7, 0]}
KINDS = HAND + ("store", "hand_t") + CHUNKED + TINY


@functools.lru_cache(maxsize=None)
def tiny_edges(n):
    g = torch.Generator().manual_seed(100 + n)
    deg = TINY_DEG[n]
    if sum(deg) == 0:
        return torch.zeros(2, 0, dtype=torch.int64)
    src = torch.cat([torch.randint(0, n, (d,), generator=g) for d in deg])
    dst = torch.repeat_interleave(torch.arange(n), torch.tensor(deg))
    ei = torch.stack([src, dst])
    return ei[:, torch.randperm(ei.size(1), generator=g)]


@functools.lru_cache(maxsize=None)
def dense_edges():
    """[2, E] int64, N = 600: the key batches of the row-group walker (tests/agg_b16_ref.py; not one of
    KINDS). Rows 8..15 have in-degree 64 with disjoint sources (groups of 4: 256 keys, the group of 8:
    512); rows 16..19 hold 64 distinct sources between them, rows 24..27 hold 65, rows 20..23 and
    28..31 add a few repeats of those; row 40 is heavy (130 entries); the other rows below 560 draw 0..6
    sources below 590; rows 560..599 are isolated and rows 590..599 are no edge's source."""
    g = torch.Generator().manual_seed(600)
    rows = {8 + t: list(range(64 * t, 64 * t + 64)) for t in range(8)}
    rows.update({16: list(range(40)), 17: list(range(20, 64)), 18: list(range(5, 15)), 19: [],
                 20: [0, 1], 21: [63, 7], 22: [], 23: [3, 3],
                 24: list(range(100, 140)), 25: list(range(130, 165)), 26: list(range(100, 110)), 27: [],
                 28: [101, 102], 29: [], 30: [], 31: [],
                 40: torch.randint(0, 590, (130,), generator=g).tolist()})
    for r in range(560):
        if r not in rows:
            rows[r] = torch.randint(0, 590, (int(torch.randint(0, 7, (1,), generator=g)),), generator=g).tolist()
    src = torch.tensor([s for r in sorted(rows) for s in rows[r]], dtype=torch.int64)
    dst = torch.tensor([r for r in sorted(rows) for _ in rows[r]], dtype=torch.int64)
    ei = torch.stack([src, dst])
    return ei[:, torch.randperm(ei.size(1), generator=g)]


@functools.lru_cache(maxsize=None)
def edges(kind):
    """(edge_index [2, E] int64, N, chunk) of a structure case. hand*: the hand graph of
    tests/test_gpu_spmm_b16.py (N = 1,003, isolated rows, duplicated edges, in-degree 64 / 65 / 700,
    a short last group), also rebuilt with chunk 4 / 16 / 200; hand_t: the hand graph reversed, so
    that the TRANSPOSE holds the rows of degree 64 / 65 / 700; store: a GraphStore batch (3 super
    nodes, explicit group starts, ranges); tinyN: N rows; dense (dense_r8: the same graph, for a plan
    of 8 rows per group): dense_edges, chunk 64."""
    from test_gpu_spmm_b16 import N_HAND, hand_edges, store_batch_host
    if kind.startswith("dense"):
        return dense_edges(), 600, 64
    if kind == "store":
        b = store_batch_host()
        return b.edge_index, int(b.num_nodes), 64
    if kind in HAND:
        return hand_edges(), N_HAND, 64
    if kind in CHUNKED:
        return hand_edges(), N_HAND, int(kind[6:])
    if kind == "hand_t":
        return hand_edges().flip(0).contiguous(), N_HAND, 64
    n = int(kind[4:])
    return tiny_edges(n), n, 64


class Struct:
    """The CSR order of a structure case, computed on the host with stable sorts (bgnn_graph_build,
    include/bgnn.h): the forward CSR is edge_index sorted by target, so a row keeps edge_index order;
    the transpose CSR is the forward CSR's entries sorted by source, so a transposed row lists its
    entries in forward-CSR order; perm_t = the forward position of each transposed entry."""

    def __init__(self, ei, n, chunk):
        E = ei.size(1)
        self.ei, self.n, self.E, self.chunk = ei, n, E, chunk
        src, dst = ei[0], ei[1]
        self.order = torch.sort(dst, stable=True).indices
        self.order_t = self.order[torch.sort(src[self.order], stable=True).indices]
        self.deg = torch.bincount(dst, minlength=n)
        self.deg_t = torch.bincount(src, minlength=n)
        self.rowptr = torch.zeros(n + 1, dtype=torch.int64)
        self.rowptr[1:] = self.deg.cumsum(0)
        self.rowptr_t = torch.zeros(n + 1, dtype=torch.int64)
        self.rowptr_t[1:] = self.deg_t.cumsum(0)
        self.col = src[self.order]
        self.col_t = dst[self.order_t]
        self.pos = torch.empty(E, dtype=torch.int64)          # forward CSR position of edge e
        self.pos[self.order] = torch.arange(E)
        self.pos_t = torch.empty(E, dtype=torch.int64)        # transpose CSR position of edge e
        self.pos_t[self.order_t] = torch.arange(E)
        self.perm_t = self.pos[self.order_t]
        self.off = self.pos - self.rowptr[dst]                # edge e's offset in its forward row
        self.off_t = self.pos_t - self.rowptr_t[src]          # ... in its transposed row
        self.row_of = torch.repeat_interleave(torch.arange(n), self.deg)   # row of each forward CSR position


@functools.lru_cache(maxsize=None)
def struct(kind):
    return Struct(*edges(kind))


# ============================================================================ the kernel geometry
def geometry(H, aligned):
    """(vec, nv, lpr, column tiles) of pick_geometry (csrc/spmm.hip), from the documented rules:
    float4 columns when every pointer is 16-byte aligned and H and every ld are multiples of 4, else
    scalar; a row takes lpr = the next power of two of its vectors in [16, 64] lanes (several rows
    per wave below 64); above 64 float4 per row a lane holds two, above 128 the columns are tiled."""
    def p2(x):
        p = 1
        while p < x:
            p *= 2
        return p
    if aligned and H % 4 == 0:
        nv4 = H // 4
        lpr, nv = (64, 2) if nv4 > 64 else (p2(max(nv4, 16)), 1)
        return 4, nv, lpr, -(-H // (lpr * 4 * nv))
    lpr = p2(min(max(H, 16), 64))
    return 1, 1, lpr, -(-H // lpr)


# (H, variant): "" = aligned pointers and ld % 4 == 0; "off4" = the source pointer 4 bytes past a
# 16-byte boundary; "ldodd" = an output ld that is no multiple of 4 -- both scalar geometries at H % 4 == 0
H_CASES = [(h, "") for h in (1, 3, 17, 33, 65, 4, 64, 68, 128, 132, 252, 256, 260, 508, 512, 516, 1024)] + \
          [(100, "off4"), (64, "ldodd")]
# the geometry each case must reach, written out by hand from the classes of DESIGN.md section 4b
EXPECT_GEOMETRY = {
    (1, ""): (1, 1, 16, 1), (3, ""): (1, 1, 16, 1), (17, ""): (1, 1, 32, 1), (33, ""): (1, 1, 64, 1),
    (65, ""): (1, 1, 64, 2), (100, "off4"): (1, 1, 64, 2), (64, "ldodd"): (1, 1, 64, 1),
    (4, ""): (4, 1, 16, 1), (64, ""): (4, 1, 16, 1), (68, ""): (4, 1, 32, 1), (128, ""): (4, 1, 32, 1),
    (132, ""): (4, 1, 64, 1), (252, ""): (4, 1, 64, 1), (256, ""): (4, 1, 64, 1),
    (260, ""): (4, 2, 64, 1), (508, ""): (4, 2, 64, 1), (512, ""): (4, 2, 64, 1),
    (516, ""): (4, 2, 64, 2), (1024, ""): (4, 2, 64, 2),
}
# the other structure cases run one H per kernel family: scalar, several rows per wave, one row per
# wave (the row-group kernel where planned), two vectors per lane, column tiles
H_SHORT = [(3, ""), (68, ""), (256, ""), (512, ""), (516, "")]


def family(H, variant, seg_kernel, chunk, grouped, reduce_is_sum_like):
    """the light-row kernel a launch takes (launch_all, csrc/spmm.hip): 'group' (row-group plan,
    SUM / MEAN / MEANT, one column tile, BGNN_TUNE_SEG_KERNEL 0), 'sweep' (one row per wave, float4,
    chunk <= 64, knob not 1) or 'blocked' (k_seg_light: everything else)"""
    vec, _nv, lpr, tiles = geometry(H, variant == "")
    full = vec == 4 and lpr == 64 and chunk <= 64
    if full and seg_kernel == 0 and grouped and reduce_is_sum_like and tiles == 1:
        return "group"
    return "sweep" if full and seg_kernel != 1 else "blocked"


# ============================================================================ inputs
def _seed(kind, H, salt):
    return (sum((i + 1) * ord(c) for i, c in enumerate(kind)) * 4099 + 31 * H + salt) % (2 ** 31 - 1)


@functools.lru_cache(maxsize=None)
def randn_rows(kind, H, salt=0):
    """f32 [N, H] standard normal, seeded per (case, H, use)"""
    n = edges(kind)[1]
    return torch.randn(n, H, generator=torch.Generator().manual_seed(_seed(kind, H, salt)))


@functools.lru_cache(maxsize=None)
def ties_rows(kind, H):
    """small integers clamped at 0 (seven of eight values are 0, the rest 1): most columns tie"""
    n = edges(kind)[1]
    g = torch.Generator().manual_seed(_seed(kind, H, 7))
    return torch.randint(-6, 2, (n, H), generator=g).clamp_min(0).float()


def nonfinite_targets(kind):
    """the rows whose columns lose every finite neighbour: the first row with edges, the first row of
    in-degree exactly chunk, the heavy row of the largest in-degree (hand: rows 0, 10 and 500)"""
    S = struct(kind)
    rows = []
    for m in (S.deg > 0, S.deg == S.chunk, (S.deg > S.chunk) & (S.deg == S.deg.max())):
        nz = m.nonzero().flatten()
        if nz.numel() and int(nz[0]) not in rows:
            rows.append(int(nz[0]))
    return rows


def nonfinite_cols(H):
    return sorted({0, H // 2, H - 1})


@functools.lru_cache(maxsize=None)
def nonfinite_rows(kind, H):
    """randn with, for each target row and a few columns, -inf (first column), NaN (second) or the two
    alternating (third) in EVERY in-neighbour, so the whole column has no winner; and one NaN among
    finite values in the second in-neighbour of another row of in-degree >= 3"""
    S = struct(kind)
    x = randn_rows(kind, H, 3).clone()
    rows = nonfinite_targets(kind)
    for r in rows:
        nb = S.col[S.rowptr[r]:S.rowptr[r + 1]]
        for i, c in enumerate(nonfinite_cols(H)):
            if i == 0:
                x[nb, c] = NEG_INF
            elif i == 1:
                x[nb, c] = float("nan")
            else:
                for k, j in enumerate(nb.tolist()):   # (a repeated source keeps its last value: still no winner)
                    x[j, c] = NEG_INF if k % 2 == 0 else float("nan")
    poisoned = torch.zeros(S.n, dtype=torch.bool)
    for r in rows:
        poisoned[S.col[S.rowptr[r]:S.rowptr[r + 1]]] = True
    for r in (S.deg >= 3).nonzero().flatten().tolist():
        nb = S.col[S.rowptr[r]:S.rowptr[r + 1]]
        if r not in rows and not bool(poisoned[nb].any()):
            x[int(nb[1]), H // 3] = float("nan")
            break
    return x


# ============================================================================ sums
def _keep(S, transposed, mut, with_addend):
    """the edges a mutated kernel still adds (bool over edge_index columns) and the rows it leaves
    unwritten (bool over rows), for the structure mutations:
      drop_last   the last entry of one row is left out: the first row of degree chunk if there is
                  one (the last lane of the one-vector col load), else the last row with edges
      drop_chunk  the second chunk of every heavy row is left out
      b65_light   a row of degree chunk + 1 treated as light: its entries past the first chunk (one
                  vector load of col) are lost
      b64_heavy   a row of degree exactly chunk treated as heavy: the light pass skips it and no
                  chunk covers it, so neither its sum nor its addend is written (modelled as 0)"""
    deg, off, tgt = (S.deg_t, S.off_t, S.ei[0]) if transposed else (S.deg, S.off, S.ei[1])
    keep = torch.ones(S.E, dtype=torch.bool)
    lost = torch.zeros(S.n, dtype=torch.bool)
    if mut == "drop_last":
        at = (deg == S.chunk).nonzero().flatten()
        r = int(at[0]) if at.numel() else int((deg > 0).nonzero().flatten()[-1])
        keep[(tgt == r) & (off == deg[r] - 1)] = False
    elif mut == "drop_chunk":
        keep[(deg[tgt] > S.chunk) & (off >= S.chunk) & (off < 2 * S.chunk)] = False
    elif mut == "b65_light":
        keep[(deg[tgt] == S.chunk + 1) & (off >= S.chunk)] = False
    elif mut == "b64_heavy":
        lost = deg == S.chunk
    return keep, lost


def sum_bound(cnt, k, mag):
    """(cnt - 1 + k) u sum |terms| per element (0 for an empty or one-term row without roundings)"""
    return (cnt.to(D).view(-1, 1) - 1 + k).clamp_min(0) * U * mag


def fwd_ref(kind, x, reduce, mut=None):
    """bgnn_spmm_fwd SUM / MEAN: out[r] = s_r sum_{e in row r} x[col[e]], s_r = 1 or 1 / max(deg, 1);
    empty rows give 0. -> (fp64 result, bound). k = 0 (SUM), 2 (MEAN: inv_deg and its product)."""
    S = struct(kind)
    keep, lost = _keep(S, False, mut, False)
    src, dst = S.ei[0][keep], S.ei[1][keep]
    t = x.to(D)[src]
    H = x.size(1)
    agg = torch.zeros(S.n, H, dtype=D).index_add_(0, dst, t)
    mag = torch.zeros(S.n, H, dtype=D).index_add_(0, dst, t.abs())
    if reduce == MEAN:
        s = (1.0 / ((S.deg + 1) if mut == "deg_plus_1" else S.deg.clamp_min(1)).to(D)).view(-1, 1)
        agg, mag = s * agg, s * mag
    agg[lost] = 0
    return agg, sum_bound(S.deg, 2 if reduce == MEAN else 0, mag)


def bwd_ref(kind, g, reduce, addend=None, mut=None):
    """bgnn_spmm_bwd / bgnn_spmm_bwd_add: gx[j] = sum_{q in rowT j} w(t_q) g[t_q] (+ addend[j]),
    w = 1 (SUM) or 1 / max(deg_fwd(t), 1) (MEAN). -> (fp64 result, bound). k = 0 (SUM), 2 (MEAN: the
    weight and the product of every term); the addend is one more term."""
    S = struct(kind)
    keep, lost = _keep(S, True, mut, addend is not None)
    src, dst = S.ei[0][keep], S.ei[1][keep]
    H = g.size(1)
    if reduce == MEAN:   # mutation: the source's out-degree in place of the target's in-degree
        w = 1.0 / (S.deg_t[src] if mut == "out_degree" else S.deg[dst]).clamp_min(1).to(D)
        t = g.to(D)[dst] * w.view(-1, 1)
    else:
        t = g.to(D)[dst]
    gx = torch.zeros(S.n, H, dtype=D).index_add_(0, src, t)
    mag = torch.zeros(S.n, H, dtype=D).index_add_(0, src, t.abs())
    cnt = S.deg_t.clone()
    if addend is not None:
        if mut != "no_addend":
            gx = gx + addend.to(D)
        mag = mag + addend.to(D).abs()
        cnt = cnt + 1
    gx[lost] = 0
    return gx, sum_bound(cnt, 2 if reduce == MEAN else 0, mag)


# ============================================================================ max
def _max_scan(S, x):
    """per forward CSR position the value a strict > compares (a NaN never wins: it compares as
    -inf), per (row, column) the maximum (-inf when no edge wins) and the hits"""
    H = x.size(1)
    v = x.to(D)[S.col]
    v = torch.where(torch.isnan(v), torch.full_like(v, NEG_INF), v)
    idx = S.row_of.view(-1, 1).expand(-1, H)
    top = torch.full((S.n, H), NEG_INF, dtype=D).scatter_reduce_(0, idx, v, "amax", include_self=True)
    hit = v == top[S.row_of]
    return v, top, hit, idx


def max_fwd_ref(kind, x, mut=None):
    """bgnn_spmm_fwd(MAX): dict(out = the maximum over the row's edges by strict > from -inf (exact;
    -inf when every neighbour is -inf or NaN; 0 for an empty row), pos = the forward CSR position of
    the first maximising edge in CSR order -- the row's first edge when no edge wins -- or -1 for an
    empty row, off = pos - rowptr[row], winner = whether an edge won). mut 'last_tie': the last
    maximising edge."""
    S = struct(kind)
    H = x.size(1)
    _v, top, hit, idx = _max_scan(S, x)
    p = torch.arange(S.E).view(-1, 1).expand(-1, H)
    if mut == "last_tie":
        pos = torch.full((S.n, H), -1, dtype=torch.int64).scatter_reduce_(
            0, idx, torch.where(hit, p, torch.full_like(p, -1)), "amax", include_self=True)
    else:
        pos = torch.full((S.n, H), S.E, dtype=torch.int64).scatter_reduce_(
            0, idx, torch.where(hit, p, torch.full_like(p, S.E)), "amin", include_self=True)
    has = (S.deg > 0).view(-1, 1).expand(-1, H)
    pos = torch.where(has, pos, torch.full_like(pos, -1))
    out = torch.where(has, top, torch.zeros((), dtype=D))
    off = torch.where(has, pos - S.rowptr[:-1].view(-1, 1), torch.zeros_like(pos))
    return dict(out=out, pos=pos, off=off, winner=has & (top > NEG_INF))


def max_bwd_ref(kind, x, g, addend=None, mut=None, fwd=None):
    """bgnn_spmm_bwd_max on the forward's state: gx[j, c] = sum of g[i, c] over the edges j -> i that
    are the argmax of (i, c) (+ addend[j, c]). -> (fp64 result, bound): the sum bound over the m
    matching edges, the addend one more term. fwd: max_fwd_ref(kind, x), when the caller holds it. mut 'last_tie' (the state's), 'split_ties' (the gradient
    divided among all maximising edges), 'no_addend'."""
    S = struct(kind)
    H = x.size(1)
    gd = g.to(D)
    if mut == "split_ties":
        _v, _top, hit, idx = _max_scan(S, x)
        nt = torch.zeros(S.n, H, dtype=D).scatter_add_(0, idx, hit.to(D))
        t = torch.where(hit, (gd / nt.clamp_min(1))[S.row_of], torch.zeros((), dtype=D))
        gx = torch.zeros(S.n, H, dtype=D).index_add_(0, S.col, t)
        mag = torch.zeros(S.n, H, dtype=D).index_add_(0, S.col, t.abs())
        m = torch.zeros(S.n, H, dtype=D).index_add_(0, S.col, hit.to(D))
    else:
        pos = (fwd if fwd is not None and mut is None else max_fwd_ref(kind, x, "last_tie" if mut == "last_tie" else None))["pos"]
        has = pos >= 0
        to = torch.where(has, S.col[pos.clamp_min(0)] if S.E else pos, torch.full_like(pos, S.n))   # row N absorbs
        z = torch.zeros(S.n + 1, H, dtype=D)
        gx = z.clone().scatter_add_(0, to, gd)[:S.n]
        mag = z.clone().scatter_add_(0, to, gd.abs())[:S.n]
        m = z.clone().scatter_add_(0, to, torch.ones_like(gd))[:S.n]
    if addend is not None:
        if mut != "no_addend":
            gx = gx + addend.to(D)
        mag = mag + addend.to(D).abs()
        m = m + 1
    return gx, (m - 1).clamp_min(0) * U * mag


def amax_ref(prev, gx, mut=None):
    """*amax = max(previous, max |gx|) over the rows written, exact in f32 (mut: without the previous)"""
    m = float(gx.abs().max()) if gx.numel() else 0.0
    return m if mut == "amax_no_prev" else max(float(torch.tensor(prev, dtype=torch.float32)), m)
