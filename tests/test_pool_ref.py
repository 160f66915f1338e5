"""CPU: the references of tests/pool_ref.py are right and the case lists have teeth.

- rank_ref (torch's stable descending sort) equals rank_rule, the pair count of include/bgnn.h evaluated
  literally, on every size case and score kind (graphs of more than 700 nodes: on LARGE_KINDS, the pair
  count being quadratic), and each graph's ranks are a permutation of 0 .. n_g - 1, the NaN kinds
  included. The worked example of the NaN order is checked value by value.
- rank_ref + select_ref equal oracle.pyg_ref.topk for ratio 0.5 and 0.3 on every case without empty
  graphs; filter_ref equals oracle.pyg_ref.filter_adj wherever every edge end is a node.
- Every mutant of the rank rule differs from rank_ref on at least one listed case; the test prints, per
  mutant, the cases that expose it. nan_blind is the rule bgnn_topk_rank had before the NaN order: the
  NaN score kinds expose it, which records that this case list would have caught it.
- The dscore bound holds for an f32 evaluation in two summation orders.
- The plan cases hold what they are for (degrees around the chunk, entry counts around the register
  chunks, no expected gmask byte equal to the window's sentinel)."""
import math

import numpy as np
import pytest
import torch

import pool_ref as P
from oracle import pyg_ref

LARGE = 700
LARGE_KINDS = ("levels4", "equal", "nan_bits")


def rank_cases():
    for case, sizes in P.RANK_SIZES.items():
        for kind in P.SCORE_KINDS:
            if max(sizes) <= LARGE or kind in LARGE_KINDS:
                yield case, sizes, kind


def test_worked_example():
    s = torch.tensor([0.3, float("nan"), 0.9, -0.0, 0.0, float("nan"), -1.0, float("inf")])
    want = torch.tensor([1, 5, 7, 2, 0, 3, 4, 6])                      # NaN first, ties by index
    rank = P.rank_ref(s, [8])
    assert torch.equal(torch.argsort(rank), want)
    assert torch.equal(P.rank_rule(s, [8]), rank)
    assert P.rank_rule(s, [8], "nan_blind").tolist() == [2, 0, 1, 3, 4, 0, 5, 0]   # ranks 6 and 7 never taken


def test_score_kinds_hold_what_they_name():
    for case, sizes in P.RANK_SIZES.items():
        n = sum(sizes)
        ptr, _ = P.graph_arrays(sizes)
        for kind in P.SCORE_KINDS:
            assert P.scores(case, kind).shape == (n,) and P.scores(case, kind).dtype == torch.float32
        nan = torch.isnan(P.scores(case, "nan_one"))
        assert [int(nan[int(ptr[b]):int(ptr[b + 1])].sum()) for b in range(len(sizes))] == [min(m, 1) for m in sizes]
        nan = torch.isnan(P.scores(case, "nan_graph"))
        assert any(m and bool(nan[int(ptr[b]):int(ptr[b + 1])].all()) for b, m in enumerate(sizes))
        if n >= 4:
            bits = P.scores(case, "nan_bits").view(torch.int32)
            assert all(bool((bits == P._i32(p)).any()) for p in P.NAN_BITS)
    s = P.scores("t4097", "levels4")
    assert bool(((s == 0) & torch.signbit(s)).any()) and bool(((s == 0) & ~torch.signbit(s)).any())
    s = P.scores("midblock", "nan_inf")
    assert bool(torch.isnan(s).any()) and bool(torch.isinf(s).any())
    assert len(set(P.scores("t4097", "random").tolist())) == 4097      # distinct


def test_rank_ref_is_the_pair_count_and_a_permutation():
    for case, sizes, kind in rank_cases():
        s = P.scores(case, kind)
        rank = P.rank_ref(s, sizes)
        assert torch.equal(rank, P.rank_rule(s, sizes)), f"{case} {kind}: torch's sort and the pair count differ"
    for case, sizes in P.RANK_SIZES.items():
        for kind in P.SCORE_KINDS:
            rank, o = P.rank_ref(P.scores(case, kind), sizes), 0
            for m in sizes:
                assert torch.equal(torch.sort(rank[o:o + m]).values, torch.arange(m, dtype=torch.int32)), f"{case} {kind}"
                o += m


@pytest.mark.parametrize("ratio", [0.5, 0.3])
def test_rank_and_select_equal_the_oracle(ratio):
    for case, sizes in P.RANK_SIZES.items():
        if 0 in sizes:
            continue
        _, batch = P.graph_arrays(sizes)
        for kind in P.SCORE_KINDS:
            s = P.scores(case, kind)
            k = (float(ratio) * torch.tensor(sizes).to(torch.float32)).ceil().to(torch.int64)
            perm, new_id, batch_out = P.select_ref(P.rank_ref(s, sizes), sizes, k)
            assert torch.equal(perm, pyg_ref.topk(s, ratio, batch)), f"{case} {kind} ratio {ratio}"
            assert torch.equal(batch_out, batch[perm])
            back = torch.full((sum(sizes),), -1, dtype=torch.int32)
            back[perm] = torch.arange(perm.numel(), dtype=torch.int32)
            assert torch.equal(new_id, back)


def test_select_k_kinds():
    sizes = P.RANK_SIZES["empty_mid"]
    assert P.k_of(sizes, "zero").tolist() == [0] * 6 and P.k_of(sizes, "all").tolist() == sizes
    assert P.k_of(sizes, "one").tolist() == [1, 0, 0, 1, 0, 1] and P.k_of(sizes, "half").tolist() == [4, 0, 0, 150, 0, 3]
    rank = P.rank_ref(P.scores("empty_mid", "random"), sizes)
    perm, new_id, batch_out = P.select_ref(rank, sizes, P.k_of(sizes, "all"))
    assert torch.equal(torch.sort(perm).values, torch.arange(sum(sizes))) and bool((new_id >= 0).all())
    perm, new_id, batch_out = P.select_ref(rank, sizes, P.k_of(sizes, "zero"))
    assert perm.numel() == 0 and bool((new_id == -1).all())


def test_filter_ref_equals_the_oracle():
    N = P.FILTER_N
    for E in P.FILTER_E:
        for kept in P.FILTER_KEPT:
            ei, new_id = P.filter_inputs(E, kept)
            out, pos, n_kept = P.filter_ref(ei, new_id, N)
            assert out.shape == (2, n_kept) and pos.shape == (n_kept,)
            want = {"none": 0, "all": E, "first": 1, "last": 1, "last_block": E - (E - 1) // 1024 * 1024}.get(kept)
            assert want is None or n_kept == want, f"E={E} {kept}: {n_kept} kept"
            if kept == "first":
                assert pos.tolist() == [0]
            if kept in ("last", "last_block"):
                assert int(pos[-1]) == E - 1 and int(pos[0]) == E - n_kept
            if kept == "half" and E >= 1023:
                assert 0.15 * E < n_kept < 0.35 * E
            if kept == "half_bad_ends":
                bad = ((ei < 0) | (ei >= N)).any(0)
                assert int(bad.sum()) == max(1, E // 100) and not bool(bad[pos].any())
                if E >= 4099:
                    assert {-1, N, 2 ** 40} <= set(ei[:, bad].flatten().tolist())
                continue
            ids = new_id.to(torch.int64)
            perm = torch.argsort(ids)[int((ids < 0).sum()):]
            o2, attr = pyg_ref.filter_adj(ei, torch.arange(E), perm, N)
            assert torch.equal(out, o2) and torch.equal(pos, attr), f"E={E} {kept}"


def test_every_mutant_of_the_rank_rule_is_exposed():
    exposed = {m: [] for m in P.RANK_MUTANTS}
    for case, sizes, kind in rank_cases():
        s = P.scores(case, kind)
        rank = P.rank_ref(s, sizes)
        for m in P.RANK_MUTANTS:
            if not torch.equal(P.rank_rule(s, sizes, m), rank):
                exposed[m].append(f"{case}/{kind}")
    print()
    for m, hits in exposed.items():
        print(f"  {m}: exposed by {len(hits)} cases: {' '.join(hits)}")
        assert hits, f"no listed case exposes the mutant {m}"
    kinds = {h.split("/")[1] for h in exposed["nan_blind"]}
    assert kinds == set(P.NAN_KINDS), f"the NaN-blind rule is exposed by {sorted(kinds)}"
    for case in P.RANK_SIZES:         # ... on every size case with a graph of more than one node
        if max(P.RANK_SIZES[case]) > 1:
            assert any(h.startswith(case + "/") for h in exposed["nan_blind"]), case
    # the tile origin shows only where a block's staged range exceeds one tile and holds adjacent ties
    assert {h.split("/")[0] for h in exposed["tile_origin"]} == {"t4097", "midblock"}


def test_dscore_bound_holds_for_two_f32_orders():
    worst = 0.0
    for H in P.GATHER_H:
        for n in P.GATHER_ROWS:
            g, x, new_id, score = P.gather_bwd_inputs(H, n, "none")
            dx, ds, bound = P.gather_scale_bwd_ref(g, x, new_id, score)
            gp = g[new_id.long()].numpy()
            prod = gp * x.numpy()                                       # f32 products, each rounded
            fwd = np.zeros(n, dtype=np.float32)
            for c in range(H):
                fwd = fwd + prod[:, c]
            lanes = np.zeros((n, 64), dtype=np.float32)                 # 64 strided partial sums, then a tree
            for c in range(H):
                lanes[:, c % 64] += prod[:, c]
            w = 64
            while w > 1:
                w //= 2
                lanes = lanes[:, :w] + lanes[:, w:2 * w]
            for got in (fwd, lanes[:, 0]):
                err = (torch.from_numpy(got).to(P.D) - ds).abs()
                assert bool((err <= bound).all()), f"H={H} n={n}"
                worst = max(worst, float((err / bound.clamp_min(1e-300)).max()))
            assert torch.equal(dx, g[new_id.long()] * score.view(-1, 1))
    assert 0.0 < worst <= 1.0
    g, x, new_id, score = P.gather_bwd_inputs(68, 9, "half")
    dx, ds, bound = P.gather_scale_bwd_ref(g, x, new_id, score)
    drop = new_id < 0
    assert int(drop.sum()) == 5 and bool((dx[drop] == 0).all()) and bool((ds[drop] == 0).all()) and bool((bound[drop] == 0).all())
    assert bool(torch.isfinite(dx).all()) and bool(torch.isfinite(ds).all()) and bool(torch.isnan(x[drop]).all())
    assert all(int((P.gather_bwd_inputs(5, n, "all")[2] >= 0).sum()) == 0 for n in P.GATHER_ROWS)


def test_gather_inputs():
    for H in P.GATHER_H:
        for K in P.GATHER_ROWS:
            x, score, perm = P.gather_inputs(H, K)
            named = torch.zeros(x.size(0), dtype=torch.bool)
            named[perm] = True
            assert int(named.sum()) == K and bool(torch.isnan(x[~named]).all()) and bool(torch.isfinite(x[named]).all())
            assert bool(torch.isfinite(P.gather_scale_ref(x, perm, score)).all())


def test_heavy_cases():
    for chunk in P.HEAVY_CHUNKS:
        cases = P.heavy_cases(chunk)
        degs = set()
        for name, rp in cases.items():
            deg = np.diff(rp)
            degs |= set(deg.tolist())
            hr, c0, owner, counts = P.heavy_plan_ref(rp, chunk)
            assert len(hr) == counts[0] and len(c0) == counts[0] + 1 and len(owner) == counts[1] == c0[-1]
            assert counts[1] <= 2 * (int(rp[-1]) // chunk) + 2          # the capacity include/bgnn.h names
            assert np.array_equal(deg[hr] > chunk, np.ones(len(hr), dtype=bool)) and int((deg > chunk).sum()) == len(hr)
            assert np.array_equal(np.diff(c0), -(-deg[hr] // chunk))
        assert degs == {0, chunk - 1, chunk, chunk + 1, 11 * chunk + 3}
        assert P.heavy_plan_ref(cases["no_heavy"], chunk)[3].tolist() == [0, 0]
        assert P.heavy_plan_ref(cases["last_heavy"], chunk)[0].tolist() == [3, 4]
        assert P.heavy_plan_ref(cases["last_heavy"], chunk)[1].tolist() == [0, 2, 2 + -(-(11 * chunk + 3) // chunk)]
        assert len(cases["R1_heavy"]) == 2 and len(cases["R257"]) == 258
        assert int(np.diff(cases["R257_last_heavy"])[-1]) == chunk + 1


def test_group_cases():
    for R, chunk in P.GROUP_CASES:
        rowptr, col, n, entries = P.group_csr(R, chunk)
        assert n % R and len(entries) == -(-n // R)
        deg = np.diff(rowptr)
        light = np.where(deg <= chunk, deg, 0)
        got = [int(light[g * R:g * R + R].sum()) for g in range(len(entries))]
        assert got == entries
        assert set(entries) >= {c for c in P.GROUP_COUNTS if c < R * chunk} | {R * chunk}
        assert int((deg > chunk).sum()) == 1
        gsrc, gmask, gcnt = P.group_plan_ref(R, chunk)
        assert int(gcnt.max()) == R * chunk and 1 in gcnt.tolist() and 0 in gcnt.tolist()   # every register chunk full
        assert any(c < e for c, e in zip(gcnt.tolist(), entries))      # shared sources: fewer keys than entries
        assert bool((np.bincount(gmask[gsrc != P.I32_SENTINEL], minlength=256)[[1 << t for t in range(R)]] > 0).all())
        grow = P.group_starts(R, chunk)
        assert grow[0] == 0 and grow[-1] == n and set(np.diff(grow).tolist()) >= set(range(1, R + 1))
        for gr in (None, grow):
            gsrc, gmask, gcnt = P.group_plan_ref(R, chunk, gr)
            written = gsrc != P.I32_SENTINEL
            assert int(written.sum()) == int(gcnt.sum())
            assert not bool((gmask[written] == P.U8_SENTINEL).any()) and bool((gmask[~written] == P.U8_SENTINEL).all())
            assert bool((gmask[written] != 0).all())
