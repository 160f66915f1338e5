"""CPU: the references of tests/agg_b16_ref.py are right and their bounds have teeth.

- The structure cases hold what they are for: the chunk counts of the combine cases (16, 17, 175 and
  44 chunks: per = 1, 2, 11, 3), the key counts of `dense` (64, 65 and 256 keys in groups of 4, 512
  in a group of 8, counts that are no multiple of the gather batch), NaN rows in every gathered
  plane where the structure has a row no edge names, and the slot counts written out per kind.
- The references equal an independent statement to 1e-12 relative on the matrix's own (poisoned)
  inputs: the sums oracle.pyg_ref.sage_aggregate and its autograd, the layer formulas a plain dense
  fp64 A @ z_l; every reference is finite in every element although the inputs carry NaN.
- The flag cycles meet every flag value on every kind and at every H.
- Every mutation moves the fp64 result by more than 8 x the bound (on the exact input: changes it at
  all, the bound being 0) on at least one case; the unmutated reference against itself gives 0. A
  mutation is skipped for a case only where it cannot show, each line says why:
    combine_floor        no row of more than 16 chunks that is no multiple of 16 (hand_c4, hand_c16 have)
    idle_wave_garbage    no heavy row, or none with an idle wave
    batch2_lost          no group of more than 64 keys (hand, hand_r8, dense, dense_r8 have; chunk 4 /
                         16 caps a group at 16 / 64 keys), or no row-group plan
    mask_tail_absorbed   no row-group plan restated on the host (no plan, or the store's own starts)
    drop_chunk / b64_heavy / b65_light / deg_plus_1 / out_degree   as in tests/test_spmm_ref.py
    mean_scales_zr       SUM does not scale; relu_then_affine / skip_inside_relu need their flag
    slot_of_wrong_row    no heavy row
  spmm_ref's no_addend and amax_no_prev have no counterpart: the bf16 entry points take neither."""
import pytest
import torch

import agg_b16_ref as A
import sage_rows_ref as SR
import spmm_ref as R
from oracle import pyg_ref

D = torch.float64
TEETH = 8.0
TEETH_H = (8, 72, 504)


def close(a, b, what):
    a, b = a.to(D), b.to(D)
    assert bool(torch.isfinite(a).all()), what + ": the reference is not finite everywhere"
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30), what


def store_groups():
    return SR.host_graph("store")[3][1]


# ----------------------------------------------------------------------------- structure
def test_combine_cases():
    c4, c16 = A.chunks_of("hand_c4"), A.chunks_of("hand_c16")
    assert (c4[10], c4[11], c4[500]) == (16, 17, 175) and c16[500] == 44
    assert A.combine_runs(16) == (1, 16)       # every wave one chunk
    assert A.combine_runs(17) == (2, 9)        # waves 9..15 idle
    assert A.combine_runs(175) == (11, 16)     # the last run clamped: 175 - 15 * 11 = 10 chunks
    assert A.combine_runs(44) == (3, 15)       # 15 runs, wave 15 idle, the last run of 2
    assert max(A.chunks_of("hand").values()) == 11 and max(A.chunks_of("store").values()) <= 16   # (what the old tests reach)
    assert A.chunks_of("hand_t", True)[500] == 11 and not A.chunks_of("hand_t")


def test_dense_key_batches():
    S = R.struct("dense")
    assert S.n == 600 and S.chunk == 64 and "dense" not in R.KINDS
    k4, g4 = A.edge_keys("dense", 4)
    k8, g8 = A.edge_keys("dense_r8", 8)
    assert {64, 65, 256} <= set(g4.tolist()) and 512 in g8.tolist()
    assert g4[2] == 256 and S.deg[8:12].tolist() == [64] * 4          # four light rows of in-degree 64,
    assert S.col[S.rowptr[8]:S.rowptr[12]].unique().numel() == 256    # disjoint sources
    assert g8[1] == 512 and g4[4] == 64 and g4[6] == 65
    assert int((g4 % 8 != 0).sum()) > 0 and int((g8 % 4 != 0).sum()) > 0 and g8[3] == 65
    assert int((k4 == -1).sum()) == 130 == int(S.deg[40])              # the heavy row's entries are no keys
    # the hand graph: only the group around row 10 exceeds one key batch
    _, gh = A.edge_keys("hand", 4)
    assert int((gh > 64).sum()) == 1 and int(gh[2]) == 67


def test_poison_rows_and_slots():
    want = {"hand": (11, 101), "hand_t": (101, 11), "store": (0, 0), "tiny1": (0, 0), "tiny3": (0, 1), "tiny5": (0, 0),
            "tiny9": (0, 1), "dense": (14, 126)}
    for kind in A.KINDS:
        base = "dense" if kind.startswith("dense") else kind if kind in want else "hand"
        got = (int(A.unnamed(kind).sum()), int(A.unnamed(kind, True).sum()))
        assert got == want[base], (kind, got)       # (store, tiny1, tiny5: every row is named in both directions)
        for tr in (False, True):
            x = A.randn_b16(kind, 8, 0, tr)
            assert int(torch.isnan(x).any(1).sum()) == got[tr]
        z = A.layer_inputs(kind, 8)["z"]
        assert int(torch.isnan(z[:, :8]).any(1).sum()) == got[0] and bool(torch.isfinite(z[:, 8:]).all())
        light, nh, groups = A.expect_slots(kind, store_groups() if kind == "store" else None)
        assert (light, nh) == A.EXPECT_SLOTS[kind]
        assert light + nh == SR.fwd_slots(R.struct(kind).n, nh, groups)
    assert A.zero_row("hand") == 900 and A.zero_row("store") is None


def test_flag_cycles_cover():
    for cases, nflags in ((A.INFER_CASES, 4), (A.FWD_CASES, 2)):
        for axis in (0, 1):
            for v in {c[0][axis] for c in cases}:
                seen = [f for c, f in cases if c[axis] == v]
                for i in range(nflags):
                    assert {f[i] for f in seen} == {0, 1}, (v, i)
    for i in range(3):
        for h in A.H_SHORT:
            assert {f[i] for (n, hh), f in A.TAIL_CASES if hh == h} == {0, 1}
        for n in SR.NS:
            assert {f[i] for (nn, hh), f in A.TAIL_CASES if nn == n} == {0, 1}
    assert len(A.CASES) == 9 + 13 * 4


def test_subbf16_rows_have_another_winner_than_their_rounding():
    for kind in ("hand", "dense", "tiny5"):
        x = A.subbf16_rows(kind, 8)
        f, r = R.max_fwd_ref(kind, x), R.max_fwd_ref(kind, x.to(A.BF).float())
        assert torch.equal(f["out"].float().to(A.BF), r["out"].float().to(A.BF))       # rounding is monotone
        differ = int((f["pos"] != r["pos"]).sum())
        assert differ > 0.1 * f["pos"].numel() * (kind != "tiny5") and differ > 0


# ----------------------------------------------------------------------------- independent statements
@pytest.mark.parametrize("kind", A.KINDS)
def test_sums_agree_with_the_oracle(kind):
    S = R.struct(kind)
    H = 8
    for xb, gb in ((A.randn_b16(kind, H, 0), A.randn_b16(kind, H, 1, True)), (A.exact_b16(kind, H), A.exact_b16(kind, H, True))):
        for reduce, aggr in ((A.SUM, "add"), (A.MEAN, "mean")):
            x = torch.nan_to_num(xb.to(D)).requires_grad_(True)         # (the oracle reads every row)
            out = pyg_ref.sage_aggregate(x, S.ei, aggr)
            close(A.sum_ref(kind, xb, reduce)[0], out.detach(), f"{kind} {aggr} forward")
            (out * torch.nan_to_num(gb.to(D))).sum().backward()
            close(A.sum_ref(kind, gb, reduce, True)[0], x.grad, f"{kind} {aggr} transpose")
    ref, bound = A.sum_ref(kind, A.exact_b16(kind, H), A.SUM)
    assert torch.equal(ref, ref.round()) and float(ref.abs().max()) < 2 ** 24 and bool(torch.isfinite(bound).all())


def dense_layer(kind, d, mean, bias):
    """the layer by a dense fp64 adjacency product"""
    S = R.struct(kind)
    H = d["z"].size(1) // 2
    Adj = torch.zeros(S.n, S.n, dtype=D).index_put_((S.ei[1], S.ei[0]), torch.ones(S.E, dtype=D), accumulate=True)
    if mean:
        Adj = Adj / Adj.sum(1, keepdim=True).clamp_min(1)
    h = Adj @ torch.nan_to_num(d["z"][:, :H].to(D)) + d["z"][:, H:].to(D) + (d["bias"].to(D) if bias else 0)
    nrm = torch.linalg.vector_norm(h, dim=1)
    return h / nrm.clamp_min(1e-12).unsqueeze(1), nrm


@pytest.mark.parametrize("kind", A.KINDS)
def test_layer_agrees_with_a_dense_product(kind):
    H = 24
    d = A.layer_inputs(kind, H)
    for mean in (0, 1):
        for bias in (0, 1):
            o, nrm = dense_layer(kind, d, mean, bias)
            L = A.layer_ref(kind, d["z"], d["bias"] if bias else None, mean)
            own = A.layer_ref(kind, d["z"], d["bias"] if bias else None, mean, "own")
            for got in (L, own):
                close(got["o"], o, f"{kind} o")
                close(got["nrm"], nrm, f"{kind} nrm")
            assert bool(torch.isfinite(L["o_bound"]).all()) and bool(torch.isfinite(L["nrm_bound"]).all())
            for affine in (0, 1):
                for skip in (0, 1):
                    y, bound = A.infer_ref(kind, d, mean, affine, skip, bias)
                    t = o * d["scale"].to(D) + d["shift"].to(D) if affine else o
                    close(y, torch.relu(t) + (d["xprev"].to(D) if skip else 0), f"{kind} y")
                    assert bool(torch.isfinite(bound).all()) and bool((bound >= 0).all())
    zr = A.zero_row(kind)
    if zr is not None:      # h = 0: o = 0 and its bound is 0, so the kernel must give ReLU(shift) + x_prev exactly
        y, bound = A.infer_ref(kind, d, 1, 1, 1, 0)
        assert float(A.layer_ref(kind, d["z"], None, 1)["nrm"][zr]) == 0.0
        assert torch.equal(y[zr], torch.relu(d["shift"].to(D)) + d["xprev"][zr].to(D))


def test_tail_is_the_layer_without_edges():
    for (n, H), (affine, skip, bias) in A.TAIL_CASES[::5]:
        d = A.tail_inputs(n, H)
        y, bound = A.tail_ref(d, affine, skip, bias)
        h = d["y"].to(D) + (d["bias"].to(D) if bias else 0)
        o = h / torch.linalg.vector_norm(h, dim=1).clamp_min(1e-12).unsqueeze(1)
        t = o * d["scale"].to(D) + d["shift"].to(D) if affine else o
        close(y, torch.relu(t) + (d["xprev"].to(D) if skip else 0), f"tail {n} x {H}")
        assert bool(torch.isfinite(bound).all())


# ----------------------------------------------------------------------------- the bounds have teeth
SHOWN = {}


def show(label, mut, r, note=""):
    print(f"{label}: {mut}: {'%.3g' % r if r is not None else 'n/a'} {note}")
    if r is not None:
        SHOWN.setdefault(mut, []).append(label)
        assert r > TEETH, f"{label}: mutation {mut} stays within {r:.3g} x the bound"


def can_show(kind, transposed, mut):
    return A.edge_weights(kind, transposed, mut)[1]


WHY = {"combine_floor": "(no row of more than 16 chunks off a multiple of 16)", "idle_wave_garbage": "(no heavy row with an idle wave)",
       "batch2_lost": "(no group of more than 64 keys, or no plan)", "mask_tail_absorbed": "(no row-group plan restated on the host)"}


@pytest.mark.parametrize("h", TEETH_H)
@pytest.mark.parametrize("kind", A.KINDS)
def test_teeth_sums(kind, h):
    S = R.struct(kind)
    for transposed, deg in ((False, S.deg), (True, S.deg_t)):
        heavy, at64, at65 = bool((deg > S.chunk).any()), bool((deg == S.chunk).any()), bool((deg == S.chunk + 1).any())
        for name, xb in (("randn", A.randn_b16(kind, h, int(transposed), transposed)), ("exact", A.exact_b16(kind, h, transposed))):
            for reduce in (A.SUM, A.MEAN):
                if name == "exact" and reduce == A.MEAN:
                    continue                                   # (the exact claim is SUM's)
                label = f"{kind} H={h} {'transpose' if transposed else 'forward'} {'mean' if reduce else 'sum'} {name}"
                true, bound = A.sum_ref(kind, xb, reduce, transposed)
                if name == "exact":
                    bound = torch.zeros_like(bound)            # bit for bit
                assert A.away(A.sum_ref(kind, xb, reduce, transposed)[0], true, bound) == 0.0

                def far(mut):
                    return A.away(A.sum_ref(kind, xb, reduce, transposed, mut)[0], true, bound)
                for mut in A.STRUCTURAL:
                    can = can_show(kind, transposed, mut)
                    show(label, mut, far(mut) if can else None, "" if can else WHY[mut])
                if name == "exact":
                    continue                                   # (an integer sum that loses a 0 does not change)
                show(label, "drop_last", far("drop_last"))
                show(label, "drop_chunk", far("drop_chunk") if heavy else None, "" if heavy else "(no heavy row)")
                for m, can in (("b64_heavy", at64), ("b65_light", at65)):
                    show(label, m, far(m) if can else None, "" if can else "(no row of that degree)")
                if reduce == A.MEAN:
                    m = "out_degree" if transposed else "deg_plus_1"
                    can = not transposed or bool((S.deg_t[S.ei[0]] != S.deg[S.ei[1]]).any())
                    show(label, m, far(m) if can else None, "" if can else "(every edge joins rows of equal degree)")


@pytest.mark.parametrize("kind", A.KINDS)
def test_teeth_max(kind):
    S = R.struct(kind)
    h = 8
    g = R.randn_rows(kind, h, 1)
    for name in ("ties", "subbf16"):
        x = A.max_input(kind, h, name)
        x = x.to(A.BF).float() if name == "ties" else x
        true, bound = R.max_bwd_ref(kind, x, g)
        assert A.away(R.max_bwd_ref(kind, x, g)[0], true, bound) == 0.0
        if int(S.ei[0].unique().numel()) <= 1:
            show(f"{kind} max {name}", "last_tie / split_ties", None, "(one source row: every edge leads to it)")
            continue
        for mut in ("last_tie", "split_ties"):
            show(f"{kind} max {name}", mut, A.away(R.max_bwd_ref(kind, x, g, None, mut)[0], true, bound))
    # the pack kernel's argmax taken on the rounded rows instead of the f32 ones
    x = A.subbf16_rows(kind, h)
    moved = bool((R.max_fwd_ref(kind, x)["pos"] != R.max_fwd_ref(kind, x.to(A.BF).float())["pos"]).any())
    true, bound = R.max_bwd_ref(kind, x, g)
    show(f"{kind} pack", "argmax_of_rounded", A.away(R.max_bwd_ref(kind, x.to(A.BF).float(), g)[0], true, bound) if moved else None,
         "" if moved else "(the f32 winner is the first of the rounded ties everywhere)")


@pytest.mark.parametrize("h", TEETH_H)
@pytest.mark.parametrize("kind", A.KINDS)
def test_teeth_layer(kind, h):
    S = R.struct(kind)
    d = A.layer_inputs(kind, h)
    nh = int((S.deg > S.chunk).sum())
    for mean in (0, 1):
        label = f"{kind} H={h} {'mean' if mean else 'sum'}"
        T = A.layer_ref(kind, d["z"], d["bias"], mean)
        assert A.away(A.layer_ref(kind, d["z"], d["bias"], mean, "own")["o"], T["o"], T["o_bound"]) < 1e-3   # (fp64 noise)

        def far(mut):
            M = A.layer_ref(kind, d["z"], d["bias"], mean, mut)
            return max(A.away(M["o"], T["o"], T["o_bound"]), A.away(M["nrm"], T["nrm"], T["nrm_bound"]))
        for mut in A.STRUCTURAL:
            can = can_show(kind, False, mut)
            show(label, mut, far(mut) if can else None, "" if can else WHY[mut])
        for mut in ("last_lane_bias", "norm_drops_lane", "zr_from_zl", "h_rounded_bf16"):
            show(label, mut, far(mut))
        can = bool(mean) and bool((S.deg >= 2).any())
        show(label, "mean_scales_zr", far("mean_scales_zr") if can else None, "" if can else "(SUM, or no row of two entries)")
        # the tail: every flag combination that can show the slip
        for affine, skip in ((1, 1), (1, 0), (0, 1)):
            true, bound = A.infer_ref(kind, d, mean, affine, skip, 1)
            assert A.away(A.infer_ref(kind, d, mean, affine, skip, 1)[0], true, bound) == 0.0
            lab = f"{label} affine={affine} skip={skip}"
            for mut in ("last_lane_bias", "norm_drops_lane", "mean_scales_zr" if can else None):
                if mut:
                    show(lab + " y", mut, A.away(A.infer_ref(kind, d, mean, affine, skip, 1, mut)[0], true, bound))
            show(lab, "relu_then_affine", A.away(A.infer_ref(kind, d, mean, affine, skip, 1, "relu_then_affine")[0], true, bound)
                 if affine else None, "" if affine else "(no scale / shift)")
            show(lab, "skip_inside_relu", A.away(A.infer_ref(kind, d, mean, affine, skip, 1, "skip_inside_relu")[0], true, bound)
                 if skip else None, "" if skip else "(no x_prev)")
        # the BatchNorm slots against the stored o
        o = T["o"].float()
        light, _nh, groups = A.expect_slots(kind, store_groups() if kind == "store" else None)
        rmax = SR.fwd_rows_per_slot(S.n, light + nh, nh, groups)
        heavy = (S.deg > S.chunk).nonzero().flatten().tolist()
        (s0, b0), (s1, b1) = A.slot_sums_ref(o, rmax, heavy)
        (m0, _), (m1, _) = A.slot_sums_ref(o, rmax, heavy, "slot_of_wrong_row")
        show(label, "slot_of_wrong_row", max(A.away(m0, s0, b0), A.away(m1, s1, b1)) if nh else None, "" if nh else "(no heavy row)")


def test_tail_teeth():
    for (n, H), (affine, skip, bias) in A.TAIL_CASES:
        d = A.tail_inputs(n, H)
        true, bound = A.tail_ref(d, affine, skip, bias)
        assert A.away(A.tail_ref(d, affine, skip, bias)[0], true, bound) == 0.0
        if affine:
            show(f"tail {n} x {H}", "relu_then_affine", A.away(A.tail_ref(d, affine, skip, bias, "relu_then_affine")[0], true, bound))
        if skip:
            show(f"tail {n} x {H}", "skip_inside_relu", A.away(A.tail_ref(d, affine, skip, bias, "skip_inside_relu")[0], true, bound))


def test_every_mutation_shows_somewhere():
    """each mutation exceeds 8 x the bound on the cases built for it"""
    SHOWN.clear()
    for kind in ("hand", "hand_t", "hand_c4", "hand_c16", "dense", "dense_r8"):
        test_teeth_sums(kind, 8)
        test_teeth_layer(kind, 504)
        test_teeth_max(kind)
    want = set(A.MUTATIONS) | {"drop_last", "drop_chunk", "deg_plus_1", "out_degree", "b64_heavy", "b65_light", "last_tie",
                               "split_ties", "argmax_of_rounded"}
    assert want <= set(SHOWN), sorted(want - set(SHOWN))

    def kinds(mut):
        return {lab.split()[0] for lab in SHOWN[mut]}
    assert {"hand_c4", "hand_c16"} <= kinds("combine_floor")
    assert {"hand", "dense", "dense_r8"} <= kinds("batch2_lost")
    assert {"hand_c4", "hand", "dense"} <= kinds("idle_wave_garbage")
    assert {"hand", "dense", "dense_r8", "hand_c4"} <= kinds("mask_tail_absorbed")
