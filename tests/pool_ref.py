"""Host references for the integer and selection kernels every SAG model and every CSR plan stands on --
csrc/pool.hip (bgnn_topk_rank, bgnn_topk_select, bgnn_gather_scale, bgnn_gather_scale_bwd,
bgnn_filter_edges) and the plan kernels of csrc/graph.hip (bgnn_heavy_plan, bgnn_group_plan): plain
torch / numpy restatements of the rules of include/bgnn.h, the inputs and the case lists shared by
tests/test_gpu_pool_matrix.py (GPU) and tests/test_pool_ref.py (CPU: agreement with the oracle,
mutants of the rank rule). No GPU is touched here.

Everything is exact (integers, or one f32 rounding per element) except dscore = <g[p], x[i]>: an H-term
sum in any order, with or without fused multiply-adds, is within gamma_H of the sum of magnitudes, so
the bound is H u sum_c |g_c x_c| with u = 2^-24 (derived, not measured).

The rank order is torch.sort(descending=True, stable=True)'s total order: -0 == +0, every NaN (any
sign, any payload) above +inf, NaNs equal among themselves, ties to the lower node index. rank_rule
states it as the pair count the kernel evaluates,
    above(a, b) = a > b or (isnan(a) and not isnan(b))
    rank[i]     = #{j > i : above(s_j, s_i)} + #{j < i : not above(s_i, s_j)}      (j in graph(i)),
and takes `mut`, one deliberate mistake of RANK_MUTANTS."""
import functools
import math

import numpy as np
import torch

from sage_rows_ref import D, U   # noqa: F401  (shared with the GPU matrix)

I32_SENTINEL = -0x5EED      # what an integer output window holds before the kernel runs
U8_SENTINEL = 0xA5

# ============================================================================ top-k rank
# graph sizes, each with the boundary it reaches (256 nodes per rank block, kRankTile = 2048 staged scores)
RANK_SIZES = {
    "one": [1],                           # one node, one lane active
    "small4": [5, 3, 1, 8],               # several graphs inside one block
    "b255_1": [255, 1],                   # a graph that ends one node before the block does
    "b256_1": [256, 1],                   # a graph that fills a block exactly; the second block holds one node
    "b257": [257],                        # one graph across two blocks
    "ones600": [1] * 600,                 # a block that touches 256 graphs
    "t2047": [2047],                      # one node short of a tile
    "t2048": [2048],                      # exactly one tile
    "t2049": [2049],                      # a second tile of one element
    "t4097": [4097],                      # three tiles, the third of one element
    "midblock": [200, 2100, 300],         # a graph that starts mid-block: the blocks' tile origins differ
    "empty_mid": [7, 0, 0, 300, 0, 5],    # graph ids without nodes, in the middle ...
    "empty_end": [9, 0],                  # ... and at the end
}
SCORE_KINDS = ("random", "levels4", "equal", "ascending", "descending", "inf",
               "nan_one", "nan_graph", "nan_bits", "nan_inf")
NAN_KINDS = ("nan_one", "nan_graph", "nan_bits", "nan_inf")
# NaNs of both signs and two payloads (the second pair are signalling NaNs)
NAN_BITS = (0x7FC00000, 0xFFC00000, 0x7FA00001, 0xFF800123)
RANK_MUTANTS = ("nan_blind", "ge_after", "ties_high", "neg_zero_below", "tile_origin")
RANK_BLOCK, RANK_TILE = 256, 2048


def graph_arrays(sizes):
    """ptr [B + 1] and batch [N], both int64, of graphs with these node counts (0 allowed)"""
    sz = torch.tensor(sizes, dtype=torch.int64)
    ptr = torch.cat([torch.zeros(1, dtype=torch.int64), sz.cumsum(0)])
    return ptr, torch.repeat_interleave(torch.arange(len(sizes)), sz)


def _i32(v):
    return v - (1 << 32) if v >= (1 << 31) else v


@functools.lru_cache(maxsize=None)
def _scores(case, kind):
    sizes = RANK_SIZES[case]
    n = sum(sizes)
    ptr, batch = graph_arrays(sizes)
    g = torch.Generator().manual_seed(1000 * sorted(RANK_SIZES).index(case) + SCORE_KINDS.index(kind))
    s = torch.randn(n, generator=g)
    nonempty = [b for b, m in enumerate(sizes) if m]
    if kind == "levels4":                 # 4 levels, the zero level with both signs
        lv = torch.tensor([-1.5, 0.0, 0.5, 2.0])[torch.randint(0, 4, (n,), generator=g)]
        neg = torch.randint(0, 2, (n,), generator=g).bool() & (lv == 0)
        s = torch.where(neg, torch.tensor(-0.0), lv)
    elif kind == "equal":
        s = torch.full((n,), 0.25)
    elif kind in ("ascending", "descending"):
        s = torch.arange(n, dtype=torch.float32) * 0.5 - 3.0
        s = s if kind == "ascending" else -s
    elif kind == "inf":
        r = torch.rand(n, generator=g)
        s = torch.where(r < 0.15, torch.tensor(float("inf")), torch.where(r > 0.85, torch.tensor(float("-inf")), s))
    elif kind == "nan_one":               # one NaN per graph
        for b in nonempty:
            s[int(ptr[b]) + int(torch.randint(0, sizes[b], (1,), generator=g))] = float("nan")
    elif kind == "nan_graph":             # a graph that is all NaN (the middle one of those with nodes)
        b = nonempty[len(nonempty) // 2]
        s[int(ptr[b]):int(ptr[b + 1])] = float("nan")
    elif kind == "nan_bits":              # about a quarter NaN, from the four bit patterns
        bits = s.view(torch.int32).clone()
        pick = torch.randint(0, 16, (n,), generator=g)
        for q, pat in enumerate(NAN_BITS):
            bits[pick == q] = _i32(pat)
        if n >= 4:                        # each pattern at least once
            where = torch.randperm(n, generator=g)[:4]
            bits[where] = torch.tensor([_i32(p) for p in NAN_BITS], dtype=torch.int32)
        s = bits.view(torch.float32)
    elif kind == "nan_inf":
        r = torch.rand(n, generator=g)
        s = torch.where(r < 0.2, torch.tensor(float("nan")), torch.where(r > 0.8, torch.tensor(float("inf")), s))
    return s.contiguous()


def scores(case, kind):
    """f32 [N] scores of a size case (shared, never written to)"""
    return _scores(case, kind)


def rank_ref(score, sizes):
    """int32 [N]: per graph, torch.sort(descending=True, stable=True) inverted to ranks"""
    score = score.detach().reshape(-1).float().cpu()
    rank = torch.empty(score.numel(), dtype=torch.int32)
    o = 0
    for m in sizes:
        if m:
            order = torch.sort(score[o:o + m], descending=True, stable=True).indices
            rank[o + order] = torch.arange(m, dtype=torch.int32)
        o += m
    assert o == score.numel()
    return rank


def _above(a, b, mut):
    """above(a, b) on numpy f32 arrays (broadcast)"""
    gt = a > b
    if mut == "neg_zero_below":           # -0 sorts below +0
        gt = gt | ((a == 0) & (b == 0) & ~np.signbit(a) & np.signbit(b))
    return gt | (np.isnan(a) & ~np.isnan(b))


def rank_rule(score, sizes, mut=None):
    """The pair count of the module text, evaluated literally (O(n_g^2)) in numpy; `mut`:
      nan_blind       the rule before the NaN order: s_j > s_i for j > i, s_j >= s_i for j < i, plain float
                      compares (all false for a NaN)
      ge_after        >= (not above(s_i, s_j)) also for j > i
      ties_high       ties go to the higher index
      neg_zero_below  -0 < +0
      tile_origin     in the staged tiles after a block's first, the split between `j < i` and `j > i` sits
                      one element early (blocks of 256 nodes; tiles of 2048 scores from the first node of
                      the block's first graph)"""
    s = score.detach().reshape(-1).float().cpu().numpy()
    ptr, batch = graph_arrays(sizes)
    ptr, batch = ptr.numpy(), batch.numpy()
    rank = np.zeros(s.size, dtype=np.int32)
    o = 0
    for m in sizes:
        if m:
            v = s[o:o + m]
            si, sj = v[:, None], v[None, :]
            idx = np.arange(m)
            after, before = idx[None, :] > idx[:, None], idx[None, :] < idx[:, None]
            if mut == "nan_blind":
                c_after, c_before = sj > si, sj >= si
            else:
                c_after, c_before = _above(sj, si, mut), ~_above(si, sj, mut)
                if mut == "ge_after":
                    c_after = ~_above(si, sj, mut)
                elif mut == "ties_high":
                    c_after, c_before = c_before, c_after
            rank[o:o + m] = (c_after & after).sum(1) + (c_before & before).sum(1)
        o += m
    if mut == "tile_origin":
        i = np.arange(1, s.size)
        lo = ptr[batch[i // RANK_BLOCK * RANK_BLOCK]]
        tie = ~_above(s[i], s[i - 1], None) & ~_above(s[i - 1], s[i], None)
        hit = (batch[i] == batch[i - 1]) & ((i - 1 - lo) // RANK_TILE >= 1) & tie
        rank[i[hit]] -= 1                 # j = i - 1 is then counted with `above`, which a tie is not
    return torch.from_numpy(rank)


# ============================================================================ top-k select
K_KINDS = ("zero", "all", "one", "half")


def k_of(sizes, kind):
    """int64 [B]: kept nodes per graph (never more than the graph holds)"""
    f = {"zero": lambda m: 0, "all": lambda m: m, "one": lambda m: min(1, m), "half": lambda m: math.ceil(0.5 * m)}[kind]
    return torch.tensor([f(m) for m in sizes], dtype=torch.int64)


def select_ref(rank, sizes, k):
    """(perm [K] int64, new_id [N] int32, batch_out [K] int64): node i is kept iff rank[i] < k[g];
    perm[new_ptr[g] + rank[i]] = i, new_id[i] = that position or -1, batch_out[position] = g"""
    _, batch = graph_arrays(sizes)
    new_ptr = torch.cat([torch.zeros(1, dtype=torch.int64), k.cumsum(0)])
    K = int(new_ptr[-1])
    r = rank.to(torch.int64)
    keep = r < k[batch]
    pos = new_ptr[batch] + r
    perm = torch.full((K,), -1, dtype=torch.int64)
    perm[pos[keep]] = torch.arange(r.numel())[keep]
    batch_out = torch.full((K,), -1, dtype=torch.int64)
    batch_out[pos[keep]] = batch[keep]
    new_id = torch.where(keep, pos, torch.tensor(-1)).to(torch.int32)
    return perm, new_id, batch_out


# ============================================================================ gather and scale
GATHER_H = (1, 4, 5, 64, 68, 260, 300, 512)   # 260: the float4 path's second trip; 300: the scalar path's fifth
GATHER_ROWS = (1, 3, 4, 5, 9)                 # 4 rows per block: one short, exact, one over, three blocks
# (name, ld - H, inputs' shift, outputs' shift), shifts in elements past a 16-byte boundary; ld = H + 1 and
# either shift force the scalar path whatever H is
GATHER_LAYOUTS = (("ld=H", 0, 0, 0), ("ld=H+4", 4, 0, 0), ("ld=H+1", 1, 0, 0), ("in+4B", 0, 1, 0), ("out+4B", 4, 0, 1))
DROP_KINDS = ("half", "all", "none")


@functools.lru_cache(maxsize=None)
def gather_inputs(H, K):
    """forward: x [N, H] with NaN in the rows perm does not name, score [N], perm [K] (distinct, unordered)"""
    g = torch.Generator().manual_seed(7000 + 16 * H + K)
    N = 2 * K + 3
    perm = torch.randperm(N, generator=g)[:K].contiguous()
    x = torch.full((N, H), float("nan"))
    x[perm] = torch.randn(K, H, generator=g)
    score = torch.full((N,), float("nan"))
    score[perm] = torch.randn(K, generator=g)
    return x, score, perm


def gather_scale_ref(x, perm, score):
    """out[p] = x[perm[p]] * score[perm[p]] in f32: one rounding per element, so bit-exact"""
    return x[perm] * score[perm].view(-1, 1)


@functools.lru_cache(maxsize=None)
def gather_bwd_inputs(H, n, drop):
    """backward: g [K, H], x [n, H] and score [n] with NaN in the dropped rows, new_id [n] int32"""
    g_ = torch.Generator().manual_seed(9000 + 64 * H + 4 * n + DROP_KINDS.index(drop))
    if drop == "half":
        keep = torch.zeros(n, dtype=torch.bool)
        keep[torch.randperm(n, generator=g_)[:n // 2]] = True     # n = 1: the one row is dropped
    else:
        keep = torch.full((n,), drop == "none")
    K = int(keep.sum())
    new_id = torch.full((n,), -1, dtype=torch.int32)
    new_id[keep] = torch.randperm(K, generator=g_).to(torch.int32)
    x = torch.full((n, H), float("nan"))
    x[keep] = torch.randn(K, H, generator=g_)
    score = torch.full((n,), float("nan"))
    score[keep] = torch.randn(K, generator=g_)
    return torch.randn(K, H, generator=g_), x, new_id, score


def gather_scale_bwd_ref(g, x, new_id, score):
    """(dx f32 [n, H], dscore fp64 [n], bound fp64 [n]): dx[i] = g[p] * score[i] (one rounding: bit-exact) and
    dscore[i] = <g[p], x[i]> with p = new_id[i]; exact zeros for dropped rows (p < 0), whose bound is 0"""
    n, H = x.shape
    keep = new_id >= 0
    p = new_id[keep].to(torch.int64)
    dx = torch.zeros(n, H)
    dx[keep] = g[p] * score[keep].view(-1, 1)
    dscore, bound = torch.zeros(n, dtype=D), torch.zeros(n, dtype=D)
    prod = g[p].to(D) * x[keep].to(D)
    dscore[keep] = prod.sum(1)
    bound[keep] = H * U * prod.abs().sum(1)
    return dx, dscore, bound


# ============================================================================ edge filter
FILTER_E = (1, 1023, 1024, 1025, 4099, 262149)   # 1024 edges per block; 262149 = 257 blocks: a second scan slice
FILTER_KEPT = ("none", "all", "half", "first", "last", "last_block", "half_bad_ends")
FILTER_N = 1000
FILTER_BLOCK = 1024


@functools.lru_cache(maxsize=None)
def filter_inputs(E, kept):
    """(edge_index [2, E] int64, new_id [N] int32): which edges survive is the case's name; half_bad_ends is
    `half` with about 1 % of the edges given an end at -1, N or 2^40"""
    N = FILTER_N
    g = torch.Generator().manual_seed(11000 + 8 * E + FILTER_KEPT.index(kept))
    if kept in ("first", "last", "last_block"):     # nodes 0 and 1 are kept, and only the named edges join them
        new_id = torch.full((N,), -1, dtype=torch.int32)
        new_id[0], new_id[1] = 1, 0
        ei = torch.randint(2, N, (2, E), generator=g)
        ei[0, :E // 2] = 0                          # one kept end is not enough
        first = {"first": 0, "last": E - 1, "last_block": (E - 1) // FILTER_BLOCK * FILTER_BLOCK}[kept]
        stop = 1 if kept == "first" else E
        ei[:, first:stop] = torch.randint(0, 2, (2, stop - first), generator=g)
        return ei, new_id
    ei = torch.randint(0, N, (2, E), generator=g)
    if kept == "none":
        new_id = torch.full((N,), -1, dtype=torch.int32)
    elif kept == "all":
        new_id = torch.randperm(N, generator=g).to(torch.int32)
    else:
        order = torch.randperm(N, generator=g)
        new_id = torch.full((N,), -1, dtype=torch.int32)
        new_id[order[:N // 2]] = torch.randperm(N // 2, generator=g).to(torch.int32)
        if kept == "half_bad_ends":
            bad = torch.tensor([-1, N, 2 ** 40])
            m = max(1, E // 100)
            pos = torch.randperm(E, generator=g)[:m]
            ei[torch.randint(0, 2, (m,), generator=g), pos] = bad[torch.randint(0, 3, (m,), generator=g)]
    return ei, new_id


def filter_ref(edge_index, new_id, N):
    """(out [2, n_kept] int64, kept [n_kept] int64, n_kept): an edge is kept iff both ends lie in [0, N) and
    map to >= 0, in edge order; out holds the relabelled ends"""
    a, b = edge_index[0], edge_index[1]
    ok = (a >= 0) & (a < N) & (b >= 0) & (b < N)
    ids = new_id.to(torch.int64)
    s = torch.where(ok, ids[a.clamp(0, max(N - 1, 0))], torch.tensor(-1))
    d = torch.where(ok, ids[b.clamp(0, max(N - 1, 0))], torch.tensor(-1))
    keep = (s >= 0) & (d >= 0)
    return torch.stack([s[keep], d[keep]]), keep.nonzero().flatten(), int(keep.sum())


# ============================================================================ heavy plan
HEAVY_CHUNKS = (1, 8, 64)


def rowptr_of(deg):
    return np.concatenate([[0], np.cumsum(np.asarray(deg, dtype=np.int64))]).astype(np.int32)


@functools.lru_cache(maxsize=None)
def heavy_cases(chunk):
    """name -> int32 rowptr: degrees from {0, chunk - 1, chunk, chunk + 1, 11 chunk + 3}"""
    c = chunk
    five = [0, c - 1, c, c + 1, 11 * c + 3]
    rng = np.random.default_rng(50 + chunk)
    return {
        "last_heavy": rowptr_of(five),                              # ends on the row of 12 chunks
        "last_light": rowptr_of([11 * c + 3, c + 1, 0, c, c - 1]),  # begins on it, ends on a light row
        "last_empty": rowptr_of([c + 1, c, 11 * c + 3, c - 1, 0]),
        "no_heavy": rowptr_of([0, c - 1, c, c, 0]),                 # counts = 0, heavy_chunk0[0] = 0
        "R1_heavy": rowptr_of([c + 1]),
        "R1_light": rowptr_of([c]),
        "R257": rowptr_of(rng.choice(five, size=257)),              # the second block of 256 rows holds one row
        "R257_last_heavy": rowptr_of(list(rng.choice(five, size=256)) + [c + 1]),
    }


def heavy_plan_ref(rowptr, chunk):
    """(heavy_row [n_heavy], heavy_chunk0 [n_heavy + 1], chunk_heavy [n_chunks], counts [2]) int32: the rows
    with deg > chunk in order, the running sum of their ceil(deg / chunk) chunks, the heavy index owning
    each chunk, and (n_heavy, n_chunks)"""
    deg = np.diff(np.asarray(rowptr, dtype=np.int64))
    heavy = np.nonzero(deg > chunk)[0]
    nch = (deg[heavy] + chunk - 1) // chunk
    c0 = np.concatenate([[0], np.cumsum(nch)])
    owner = np.repeat(np.arange(len(heavy)), nch)
    i32 = np.int32
    return heavy.astype(i32), c0.astype(i32), owner.astype(i32), np.array([len(heavy), int(nch.sum())], dtype=i32)


# ============================================================================ group plan
GROUP_CASES = ((4, 16), (8, 16), (4, 64), (8, 64))   # k_group_plan<1 / 2 / 4 / 8>: R * chunk = 64, 128, 256, 512
GROUP_COUNTS = (0, 1, 63, 64, 65, 128, 129)          # entries of a group, around the 64-entry register chunks


def np_groups(rowptr, col, n, chunk, R, grow=None):
    """Host restatement of bgnn_group_plan's rule (include/bgnn.h): per group of at most R rows
    (rows [g*R, g*R+R), or [grow[g], grow[g+1])), the light rows' entries keyed by (source,
    occurrence within the row), numbered by first appearance, with the mask of the rows holding
    each key."""
    if grow is None:
        grow = list(range(0, n, R)) + [n]
    G = len(grow) - 1
    gsrc, gmask, gcnt = {}, {}, np.zeros(G, dtype=np.int64)
    for g in range(G):
        keys, src, mask = {}, [], []
        for t in range(grow[g + 1] - grow[g]):
            r = grow[g] + t
            b, e = int(rowptr[r]), int(rowptr[r + 1])
            if e - b > chunk:
                continue
            occ = {}
            for q in range(b, e):
                s_ = int(col[q])
                k = (s_, occ.get(s_, 0))
                occ[s_] = k[1] + 1
                if k not in keys:
                    keys[k] = len(src)
                    src.append(s_)
                    mask.append(0)
                mask[keys[k]] |= 1 << t
        base = int(rowptr[grow[g]])
        for i, (s_, m) in enumerate(zip(src, mask)):
            gsrc[base + i], gmask[base + i] = s_, m
        gcnt[g] = len(src)
    return gsrc, gmask, gcnt


@functools.lru_cache(maxsize=None)
def group_csr(R, chunk):
    """(rowptr int32 [n + 1], col int32 [nnz], n, entries): a CSR whose groups of R rows hold, in order,
      - every count of GROUP_COUNTS that fits and R * chunk (each row full), the rows filled front to back,
        three times: with sources all distinct (as many keys as entries; R * chunk keys fill every register
        chunk), drawn from a pool half as large (sources shared between the rows of the group, duplicated
        edges inside a row), and all equal to one source (keys = the longest row's entries);
      - a heavy row (chunk + 5 entries) in the middle of a group, between light rows that share sources;
      - two last rows, so that n is no multiple of R.
    `entries` lists the light-entry count of each group of R rows."""
    rng = np.random.default_rng(100 * R + chunk)
    full = R * chunk
    rows, entries = [], []
    for T in [c for c in GROUP_COUNTS if c < full] + [full]:
        for flavour in ("distinct", "shared", "one"):
            pool = {"distinct": None, "shared": rng.choice(900, size=max(1, T // 2), replace=False), "one": [7]}[flavour]
            srcs = rng.permutation(900)[:T] if pool is None else rng.choice(pool, size=T)
            left, at = T, 0
            for _ in range(R):
                d = min(chunk, left)
                rows.append(list(srcs[at:at + d]))
                at, left = at + d, left - d
            entries.append(T)
    mid = [[3, 4, 5], list(rng.integers(0, 900, size=chunk + 5)), [4, 4, 9], [5, 3]] + [[] for _ in range(R - 4)]
    rows += mid
    entries.append(8)
    rows += [[1, 2, 1], [2]]
    entries.append(4)
    rowptr = rowptr_of([len(r) for r in rows])
    col = np.array([s for r in rows for s in r], dtype=np.int32)
    return rowptr, col, len(rows), entries


@functools.lru_cache(maxsize=None)
def group_starts(R, chunk):
    """explicit group starts over group_csr's rows: groups of 1 to R rows, every size at least once"""
    n = group_csr(R, chunk)[2]
    rng = np.random.default_rng(7 * R + chunk)
    grow, sizes = [0], list(range(1, R + 1))
    while grow[-1] < n:
        s = sizes.pop() if sizes else int(rng.integers(1, R + 1))
        grow.append(min(n, grow[-1] + s))
    return grow


def group_plan_ref(R, chunk, grow=None):
    """(gsrc int32 [nnz], gmask uint8 [nnz], gcnt int32 [G]) as the windows must read after the kernel ran:
    the sentinels wherever bgnn_group_plan writes nothing (behind a group's gcnt[g] keys)"""
    rowptr, col, n, _ = group_csr(R, chunk)
    s, m, cnt = np_groups(rowptr, col, n, chunk, R, grow)
    gsrc = np.full(len(col), I32_SENTINEL, dtype=np.int32)
    gmask = np.full(len(col), U8_SENTINEL, dtype=np.uint8)
    for pos, v in s.items():
        gsrc[pos], gmask[pos] = v, m[pos]
    return gsrc, gmask, cnt.astype(np.int32)
