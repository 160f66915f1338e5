"""CPU: the references of tests/spmm_ref.py are right and their bounds have teeth.

- Each formula reference equals oracle.pyg_ref.sage_aggregate (fp64) and its autograd to 1e-12
  relative: SUM / MEAN forward, their transposes (the gradient with respect to x of <out, g>), the
  transposes plus an addend, the MAX value and the MAX backward with the first-occurrence convention
  (_ScatterMaxFirst), on every structure case.
- The host CSR order is the edge_index order within each forward row and the forward-CSR order
  within each transposed row (stable sorts), and perm_t maps the transposed entries onto the forward ones.
- The geometry restated from the documented rules reaches the family each H of the matrix is meant for.
- The ties inputs tie in most (row, column) pairs; the non-finite inputs leave the intended columns
  without a winner, and the reference then names the row's first edge.
- Every mutation moves the fp64 result by more than 8 x the bound on at least one case (the ratio
  tests/test_sage_rows_ref.py requires); the unmutated result against itself stays at 0. A mutation
  is skipped for a case only where it cannot show, each line says why:
    drop_chunk / b64_heavy / b65_light   the case has no row of that degree in that direction (the
                                         hand graph's transpose has no row above 8 entries or so:
                                         hand_t carries those rows; chunk 4 / 16 / 200 move the classes)
    deg_plus_1 / out_degree              SUM does not scale
    last_tie / split_ties                randn inputs do not tie
    drop_last on the ties inputs is not run: an integer sum that loses a 0 does not change."""
import pytest
import torch

import spmm_ref as R
from oracle import pyg_ref

D = torch.float64
TEETH = 8.0
CASES = [k for k in R.KINDS]
H = 12


def close(a, b, what):
    a, b = a.to(D), b.to(D)
    assert float((a - b).abs().max()) <= 1e-12 * max(float(b.abs().max()), 1e-30), what


def test_csr_order_is_the_stable_one():
    for kind in CASES:
        S = R.struct(kind)
        src, dst = S.ei[0], S.ei[1]
        assert torch.equal(dst[S.order], torch.sort(dst).values) and torch.equal(src[S.order_t], torch.sort(src).values)
        same = dst[S.order][1:] == dst[S.order][:-1]             # inside a forward row the edge ids increase,
        assert bool((S.order[1:] > S.order[:-1])[same].all())
        same = src[S.order_t][1:] == src[S.order_t][:-1]         # inside a transposed row the forward positions
        assert bool((S.perm_t[1:] > S.perm_t[:-1])[same].all())
        assert torch.equal(S.col[S.perm_t], src[S.order_t]) and torch.equal(S.row_of[S.perm_t], S.col_t)
        assert int(S.rowptr[-1]) == S.E == int(S.rowptr_t[-1])
        assert bool((S.off >= 0).all()) and bool((S.off < S.deg[dst]).all())


def test_structure_cases_hold_what_they_are_for():
    S = R.struct("hand")
    assert (int(S.deg[10]), int(S.deg[11]), int(S.deg[500]), int((S.deg == 0).sum())) == (64, 65, 700, 101)
    assert int(S.deg_t.max()) <= 64          # the hand graph's transpose has no heavy row ...
    T = R.struct("hand_t")                   # ... its reverse does
    assert (int(T.deg_t[10]), int(T.deg_t[11]), int(T.deg_t[500])) == (64, 65, 700)
    for kind, n in zip(R.TINY, (1, 3, 5, 9)):
        assert R.struct(kind).n == n < 16
    assert int(R.struct("tiny3").deg[-1]) == 0 and int(R.struct("tiny9").deg[-1]) == 0
    assert int(R.struct("tiny5").deg.max()) == 70
    st = R.struct("store")
    assert int((st.deg > 64).sum()) == 3 and int((st.deg_t > 64).sum()) == 3 and st.n <= 1003
    assert R.struct("hand_c200").chunk == 200 and int((S.deg > 200).sum()) == 1 and int(((S.deg > 64) & (S.deg <= 200)).sum()) == 1
    assert R.nonfinite_targets("hand") == [0, 10, 500]


def test_geometry_reaches_every_family():
    assert set(R.H_CASES) == set(R.EXPECT_GEOMETRY)
    for (h, var), want in R.EXPECT_GEOMETRY.items():
        assert R.geometry(h, var == "") == want, (h, var)
    assert {g[:3] for g in R.EXPECT_GEOMETRY.values()} == {(4, 2, 64), (4, 1, 64), (4, 1, 32), (4, 1, 16), (1, 1, 64),
                                                           (1, 1, 32), (1, 1, 16)}   # the seven geometries
    assert R.family(256, "", 0, 64, True, True) == "group" and R.family(256, "", 0, 64, True, False) == "sweep"
    assert R.family(516, "", 0, 64, True, True) == "sweep" and R.family(512, "", 1, 64, True, True) == "blocked"
    assert R.family(512, "", 2, 200, False, True) == "blocked"      # a chunk above 64: no one-vector col load
    assert R.family(128, "", 2, 64, True, True) == "blocked" and R.family(100, "off4", 0, 64, True, True) == "blocked"


# ----------------------------------------------------------------------------- references vs the oracle
@pytest.mark.parametrize("kind", CASES)
def test_references_agree_with_the_oracle(kind):
    S = R.struct(kind)
    q = torch.Generator().manual_seed(17)
    x32, g32, a32 = (torch.randn(S.n, H, generator=q) for _ in range(3))
    for reduce, aggr in ((R.SUM, "add"), (R.MEAN, "mean")):
        x = x32.to(D).requires_grad_(True)
        out = pyg_ref.sage_aggregate(x, S.ei, aggr)
        close(R.fwd_ref(kind, x32, reduce)[0], out.detach(), f"{kind} {aggr} forward")
        (out * g32.to(D)).sum().backward()
        close(R.bwd_ref(kind, g32, reduce)[0], x.grad, f"{kind} {aggr} transpose")
        close(R.bwd_ref(kind, g32, reduce, a32)[0], x.grad + a32.to(D), f"{kind} {aggr} transpose + addend")
    for name, xin in (("randn", x32), ("ties", R.ties_rows(kind, H))):
        x = xin.to(D).requires_grad_(True)
        out = pyg_ref.sage_aggregate(x, S.ei, "max")
        ref = R.max_fwd_ref(kind, xin)
        assert torch.equal(ref["out"], out.detach()), f"{kind} max forward ({name})"
        (out * g32.to(D)).sum().backward()
        close(R.max_bwd_ref(kind, xin, g32)[0], x.grad, f"{kind} max backward ({name})")
        close(R.max_bwd_ref(kind, xin, g32, a32)[0], x.grad + a32.to(D), f"{kind} max backward + addend ({name})")
        # the argmax really is a maximiser, and the first one of its row
        has = ref["pos"] >= 0
        assert bool((has == (S.deg > 0).view(-1, 1)).all())
        if S.E:
            c = torch.arange(H).view(1, -1).expand(S.n, -1)
            val = xin.to(D)[S.col[ref["pos"].clamp_min(0)], c]
            assert bool((val == ref["out"])[has].all())
            assert bool((ref["off"] >= 0).all()) and bool((ref["off"] < S.deg.clamp_min(1).view(-1, 1)).all())


# ----------------------------------------------------------------------------- the special inputs
@pytest.mark.parametrize("kind", ["hand", "store", "hand_t", "tiny5"])
def test_ties_inputs_tie_in_most_pairs(kind):
    S = R.struct(kind)
    for h in (3, 64):
        _v, _top, hit, idx = R._max_scan(S, R.ties_rows(kind, h))
        nt = torch.zeros(S.n, h, dtype=D).scatter_add_(0, idx, hit.to(D))
        pairs = (S.deg > 0).view(-1, 1).expand(-1, h)
        share = float((nt[pairs] >= 2).double().mean())
        print(f"{kind} H={h}: {share:.3f} of the (row, column) pairs with edges tie")
        assert share > 0.5
        assert R.away(R.max_bwd_ref(kind, R.ties_rows(kind, h), R.randn_rows(kind, h, 1), mut="last_tie")[0],
                      *R.max_bwd_ref(kind, R.ties_rows(kind, h), R.randn_rows(kind, h, 1))) > TEETH


@pytest.mark.parametrize("h", [1, 3, 64, 516])
@pytest.mark.parametrize("kind", ["hand", "store", "hand_c200", "tiny5"])
def test_nonfinite_inputs_leave_columns_without_a_winner(kind, h):
    S = R.struct(kind)
    x = R.nonfinite_rows(kind, h)
    ref = R.max_fwd_ref(kind, x)
    rows, cols = R.nonfinite_targets(kind), R.nonfinite_cols(h)
    assert len(rows) >= 2 or kind.startswith("tiny")
    for r in rows:
        nb = S.col[S.rowptr[r]:S.rowptr[r + 1]]
        for c in cols:
            assert not bool(torch.isfinite(x[nb, c]).any())
            assert float(ref["out"][r, c]) == R.NEG_INF and not bool(ref["winner"][r, c])
            assert int(ref["off"][r, c]) == 0 and int(ref["pos"][r, c]) == int(S.rowptr[r])   # the row's first edge
    assert int((x == R.NEG_INF).sum()) > 0 and (h < 3 or int(torch.isnan(x).sum()) > 0)   # (H = 1: the -inf column alone)
    assert not bool(torch.isnan(ref["out"]).any())          # a NaN never wins
    lone = torch.isnan(x[:, h // 3]).nonzero().flatten()
    assert lone.numel() >= 1 or kind in R.TINY   # (tiny5: every one of the 5 nodes feeds a target row)
    # everywhere else an edge wins and the state points at a maximiser
    c = torch.arange(h).view(1, -1).expand(S.n, -1)
    val = x.to(D)[S.col[ref["pos"].clamp_min(0)], c]
    assert bool((val == ref["out"])[ref["winner"]].all())
    assert bool((ref["out"][(S.deg > 0) & ~ref["winner"].any(1)] == R.NEG_INF).all())
    # the gradient of a column without a winner goes to the first edge, nowhere else
    g = R.randn_rows(kind, h, 1)
    gx, _ = R.max_bwd_ref(kind, x, g)
    assert bool(torch.isfinite(gx).all())
    close(gx.sum(0), g.to(D)[S.deg > 0].sum(0), "every (row, column) with edges routes its gradient exactly once")


# ----------------------------------------------------------------------------- the bounds have teeth
SHOWN = {}


def show(label, mut, r, note=""):
    print(f"{label}: {mut}: {'%.3g' % r if r is not None else 'n/a'} {note}")
    if r is not None:
        SHOWN[mut] = max(SHOWN.get(mut, 0.0), r)
        assert r > TEETH, f"{label}: mutation {mut} stays within {r:.3g} x the bound"


@pytest.mark.parametrize("h", [3, 68, 516])
@pytest.mark.parametrize("kind", CASES)
def test_teeth(kind, h):
    S = R.struct(kind)
    x, g, a = R.randn_rows(kind, h, 0), R.randn_rows(kind, h, 1), R.randn_rows(kind, h, 2)
    xt = R.ties_rows(kind, h)
    for transposed, deg in ((False, S.deg), (True, S.deg_t)):
        heavy, at64, at65 = bool((deg > S.chunk).any()), bool((deg == S.chunk).any()), bool((deg == S.chunk + 1).any())
        for reduce in (R.SUM, R.MEAN):
            label = f"{kind} H={h} {'transpose' if transposed else 'forward'} {'mean' if reduce else 'sum'}"

            def run(mut=None, addend=None):
                return R.bwd_ref(kind, g, reduce, addend, mut) if transposed else R.fwd_ref(kind, x, reduce, mut)
            true, bound = run()
            assert R.away(run()[0], true, bound) == 0.0
            show(label, "drop_last", R.away(run("drop_last")[0], true, bound))
            show(label, "drop_chunk", R.away(run("drop_chunk")[0], true, bound) if heavy else None, "" if heavy else "(no heavy row)")
            if transposed:
                ta, ba = run(None, a)
                show(label, "no_addend", R.away(run("no_addend", a)[0], ta, ba))
                for m, can in (("b64_heavy", at64), ("b65_light", at65)):   # with an addend of their own
                    a2 = R.randn_rows(kind, h, 5)
                    t2, b2 = run(None, a2)
                    show(label, m, R.away(run(m, a2)[0], t2, b2) if can else None, "" if can else "(no row of that degree)")
            else:
                for m, can in (("b64_heavy", at64), ("b65_light", at65)):
                    show(label, m, R.away(run(m)[0], true, bound) if can else None, "" if can else "(no row of that degree)")
            if reduce == R.MEAN:
                m = "out_degree" if transposed else "deg_plus_1"
                can = not transposed or bool((S.deg_t[S.ei[0]] != S.deg[S.ei[1]]).any())
                show(label, m, R.away(run(m)[0], true, bound) if can else None,
                     "" if can else "(every edge joins a source and a target of equal degree)")
            else:
                show(label, "deg_plus_1 / out_degree", None, "(SUM does not scale)")
    label = f"{kind} H={h} max"
    for name, xin in (("randn", x), ("ties", xt)):
        ref = R.max_fwd_ref(kind, xin)
        mutd = R.max_fwd_ref(kind, xin, "last_tie")
        differ = int((mutd["pos"] != ref["pos"]).sum())
        assert torch.equal(mutd["out"], ref["out"])
        true, bound = R.max_bwd_ref(kind, xin, g, a)
        assert R.away(R.max_bwd_ref(kind, xin, g, a)[0], true, bound) == 0.0
        show(label + " " + name, "no_addend", R.away(R.max_bwd_ref(kind, xin, g, a, "no_addend")[0], true, bound))
        if name == "ties" and int(S.ei[0].unique().numel()) <= 1:
            show(label + " ties", "last_tie / split_ties", None, "(one source row: every edge leads to it)")
        elif name == "ties":
            assert differ > 0
            show(label + " ties", "last_tie", R.away(R.max_bwd_ref(kind, xin, g, a, "last_tie")[0], true, bound))
            show(label + " ties", "split_ties", R.away(R.max_bwd_ref(kind, xin, g, a, "split_ties")[0], true, bound))
        elif name == "randn":
            show(label + " randn", "last_tie / split_ties", None, "(randn inputs tie only on a repeated source)")
    for prev in (0.0, 3.0e30):
        want = R.amax_ref(prev, true.float())
        got = R.amax_ref(prev, true.float(), "amax_no_prev")
        if prev > 0:
            assert want == float(torch.tensor(prev, dtype=torch.float32)) and got != want   # exact: any difference fails
            SHOWN["amax_no_prev"] = float("inf")
        else:
            assert got == want == float(true.float().abs().max())


def test_every_mutation_shows_somewhere():
    """each mutation of the list exceeds 8 x the bound on the hand graph or its reverse"""
    SHOWN.clear()
    for kind in ("hand", "hand_t"):
        test_teeth(kind, 68)
    assert set(R.MUTATIONS) <= set(SHOWN), sorted(set(R.MUTATIONS) - set(SHOWN))
