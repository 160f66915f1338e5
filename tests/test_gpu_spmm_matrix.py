"""GPU: fp64 conformance matrix of the f32 aggregation entry points with the plain epilogue --
bgnn_spmm_fwd (SUM / MEAN / MAX, arg NULL and non-NULL), bgnn_spmm_bwd (with and without amax,
heavy_done), bgnn_spmm_bwd_add, bgnn_spmm_bwd_max (with and without an addend) and the argmax state
between them, which bgnn_spmm_max_bf16 writes too -- each on its raw entry point (_lib.call).

References, bounds, inputs, structure cases and the expected kernel geometry are
tests/spmm_ref.py's (fp64 evaluations of the header's formulas in the host's own stable CSR order;
bounds from operation counts, u = 2^-24, none measured). The device CSR is first compared with the
host's (rowptr / col / perm_t). Outputs are NaN-filled windows inside guarded allocations with
ld = ceil4(H) + 4 (guard rows and padding must survive), inputs have ld > H and NaN after their last
row and in their padding, the chunk scratch starts as NaN, the argmax state as a byte pattern with
guard bytes behind it. Every element of every output is checked; nothing is excluded.

For every H the kernel family a launch takes is asserted from bgnn_get_tuning and the documented
rules (R.family) against the family the case is meant for, so a case cannot land on another path:
scalar columns (H = 1, 3, 17, 33, 65; 100 behind a pointer 4 bytes off; 64 with an odd ld), float4
with several rows per wave (4, 64, 68, 128), one row per wave with one (132, 252, 256) or two
(260, 508, 512) vectors per lane, column tiles (516, 1024). Where the header promises bit-identity
(blocked = sweep for every U; NT and ROWS_REV change nothing) the comparison is torch.equal; the
row-group kernel is held to the bound and its first row per group is bit-identical.

After every MAX forward the state is decoded on the host and checked (offsets < deg, heavy markers,
heavy_of, arg_h in range, the offset = the reference's first maximiser, the value at it bitwise the
output) BEFORE any backward is launched with it: a forward that regresses fails on the host and
never feeds a bad state to bgnn_spmm_bwd_max. Each test runs its first configuration twice and
compares bits. Each section prints its largest err / bound."""
import pytest
import torch

import spmm_ref as R
from bgnn import _lib
from bgnn.graph import Csr, Graph, Plan, _stream
from matrix_util import RATIOS, In, Out, amax_prev, check, check_amax, ptr, scalar
from test_gpu_spmm_b16 import graph_case

pytestmark = pytest.mark.gpu

D = torch.float64
KNOBS = (1, 3, 4, 13)   # BGNN_TUNE_SEG_KERNEL, BGNN_TUNE_SEG_U, BGNN_TUNE_SEG_NT, BGNN_TUNE_ROWS_REV
SUM, MEAN, MAX = R.SUM, R.MEAN, R.MAX
_defaults = {}


@pytest.fixture(autouse=True)
def _restore_knobs():
    for k in KNOBS:
        if k not in _defaults:
            _defaults[k] = _lib.query("bgnn_get_tuning", k)
    yield
    for k in KNOBS:
        _lib.call("bgnn_set_tuning", k, _defaults[k])
    try:
        torch.cuda.synchronize()
    except RuntimeError as e:   # a device fault is sticky: nothing more of this session runs on the GPU
        pytest.exit(f"GPU fault in the aggregation matrix, session ended: {e}", returncode=3)


@pytest.fixture(scope="module", autouse=True)
def _print_ratios():
    yield
    print("\nsection: largest err / bound")
    for k in sorted(RATIOS):
        if k.startswith("spmm"):
            print(f"  {k}: {RATIOS[k]:.3f}")


# ============================================================================ structure on the device
_dev = {}


def dev_graph(kind, dev):
    """the device CSRs of a structure case (built once), after comparing them with the host's"""
    if kind in _dev:
        return _dev[kind]
    S = R.struct(kind)
    if kind in R.HAND or kind == "store":
        _ei, n, fwd, bwd, frp, g = graph_case(kind, dev)
        perm_t = g.perm_t
    else:
        g = Graph.build(S.ei.to(dev), S.n, S.chunk)
        n, fwd, bwd, frp, perm_t = S.n, g.fwd, g.bwd, g.fwd.rowptr, g.perm_t
    assert n == S.n and fwd.nnz == S.E and fwd.plan.chunk == S.chunk == bwd.plan.chunk
    for c, rp, col, what in ((fwd, S.rowptr, S.col, "forward"), (bwd, S.rowptr_t, S.col_t, "transpose")):
        assert torch.equal(c.rowptr.cpu().long(), rp), f"{kind}: {what} rowptr differs from the host's stable sort"
        assert torch.equal(c.col[:S.E].cpu().long(), col), f"{kind}: {what} col differs from the host's stable sort"
        deg = rp[1:] - rp[:-1]
        nh = int((deg > S.chunk).sum())
        assert c.plan.n_heavy == nh and c.plan.n_chunks == int((-(-deg[deg > S.chunk] // S.chunk)).sum())
        assert torch.equal(c.plan.heavy_row[:nh].cpu().long(), (deg > S.chunk).nonzero().flatten())
    assert torch.equal(perm_t[:S.E].cpu().long(), S.perm_t), f"{kind}: perm_t differs from the host's"
    rows = {"hand": 4, "hand_r8": 8, "hand_nogroups": 0, "hand_c200": 0}.get(kind, 4)
    for c in (fwd, bwd):
        assert (c.groups.rows if c.groups is not None else 0) == rows, f"{kind}: row-group plan of {rows} rows expected"
    _dev[kind] = dict(n=n, fwd=fwd, bwd=bwd, frp=frp, perm_t=perm_t, S=S, kind=kind)
    return _dev[kind]


def group_heads(csr, n):
    """first row of every row group"""
    gr = csr.groups
    return gr.grow[:gr.n_groups].cpu().long() if gr.grow is not None else torch.arange(0, n, gr.rows)


# ============================================================================ knobs and families
def configs(kind, hv, full):
    vec, _nv, lpr, _t = R.geometry(hv[0], hv[1] == "")
    if not (vec == 4 and lpr == 64):
        return [dict(k=0), dict(k=1)]          # one kernel whatever the knob says
    if full:
        return [dict(k=0), dict(k=1), dict(k=2, u=8), dict(k=2, u=12), dict(k=2, u=16), dict(k=2, nt=0), dict(k=0, rev=1),
                dict(k=0, nt=0)]
    return [dict(k=0), dict(k=1), dict(k=2)]


def set_knobs(k=0, u=0, nt=1, rev=0):
    _lib.call("bgnn_set_tuning", 1, k)
    _lib.call("bgnn_set_tuning", 3, u)
    _lib.call("bgnn_set_tuning", 4, nt)
    _lib.call("bgnn_set_tuning", 13, (_defaults[13] & ~8) | (8 if rev else 0))


# the family each H class of the hand graph (row groups of 4, chunk 64) is meant for:
# (knob 0 and a sum, knob 0 and a max, knob 1, knob 2)
def meant_family(kind, hv, k, sumlike):
    h, var = hv
    if var or h < 132 or kind == "hand_c200":      # scalar, several rows per wave, or a chunk above 64
        return "blocked"
    if k == 1:
        return "blocked"
    if k == 0 and sumlike and h <= 512 and kind != "hand_nogroups":
        return "group"
    return "sweep"


def family_of(G, csr, hv, cfg, sumlike):
    """the family of the launch to come, from the knob as the library reports it and the documented rules"""
    k = _lib.query("bgnn_get_tuning", 1)
    assert k == cfg.get("k", 0) and _lib.query("bgnn_get_tuning", 3) == cfg.get("u", 0)
    fam = R.family(hv[0], hv[1], k, csr.plan.chunk, csr.groups is not None, sumlike)
    want = meant_family(G["kind"], hv, k, sumlike)
    assert fam == want, f"{G['kind']} H={hv}: this case is meant for the {want} kernel, the rules give {fam}"
    assert R.geometry(hv[0], hv[1] == "") == R.EXPECT_GEOMETRY[hv]
    return fam


def exact_claims(results, G, csr, label):
    """results: [(family, cfg, output)]. blocked and sweep agree bit for bit for every U and NT; the
    row-group kernel agrees with itself under NT and ROWS_REV, and with the sweep on the first row of
    every group and on the heavy rows"""
    by = {}
    for fam, cfg, o in results:
        by.setdefault("group" if fam == "group" else "rows", []).append((cfg, o))
    for fam, runs in by.items():
        for cfg, o in runs[1:]:
            assert torch.equal(o.view(torch.int32), runs[0][1].view(torch.int32)), \
                f"{label}: {fam} kernel, knobs {cfg} differ in bits from knobs {runs[0][0]}"
    if "group" in by and "rows" in by:
        S = G["S"]
        deg = csr.rowptr.cpu().long()
        deg = deg[1:] - deg[:-1]
        same = torch.zeros(G["n"], dtype=torch.bool)
        same[group_heads(csr, G["n"])] = True
        same |= deg > S.chunk
        a, b = by["group"][0][1], by["rows"][0][1]
        assert torch.equal(a[same].view(torch.int32), b[same].view(torch.int32)), \
            f"{label}: the first row of a group (or a heavy row) differs in bits between the row-group and the row kernels"


# ============================================================================ runners
def scratch_for(dev, csr, H, planes=1):
    return Out(dev, 1, max(csr.plan.n_chunks, 1) * H * planes)


def windows(dev, t, hv):
    """(input, output ld): off4 moves the source 4 bytes off its alignment, ldodd makes the output ld odd"""
    return In(dev, t, lead=1 if hv[1] == "off4" else 0), (hv[0] + 3 if hv[1] == "ldodd" else None)


class ArgState:
    """the argmax state buffer: a byte pattern, 64 guard bytes behind it"""

    def __init__(self, dev, n, H, nh):
        self.n, self.H, self.nh = n, H, nh
        self.bytes = _lib.query("bgnn_spmm_max_arg_bytes", n, H, nh)
        self.hoff = (n * H + 255) // 256 * 256
        self.aoff = self.hoff + (n * 4 + 255) // 256 * 256
        assert self.bytes == self.aoff + nh * H * 4
        self.buf = torch.full((self.bytes + 64,), 0xA5, dtype=torch.uint8, device=dev)
        self.ptr = self.buf.data_ptr()

    def decode(self, label):
        b = self.buf.cpu()
        n, H, nh = self.n, self.H, self.nh
        for lo, hi, what in ((n * H, self.hoff, "padding after the byte plane"),
                             (self.hoff + 4 * n, self.aoff, "padding after heavy_of"), (self.bytes, self.bytes + 64, "guard")):
            assert bool((b[lo:hi] == 0xA5).all()), f"{label}: argmax state {what} overwritten"
        return (b[:n * H].view(n, H).long(), b[self.hoff:self.hoff + 4 * n].clone().view(torch.int32).long(),
                b[self.aoff:self.aoff + 4 * nh * H].clone().view(torch.int32).view(nh, H).long())


def check_state(state, S, csr, x, out, ref, label):
    """the safety property: a valid state, equal to the reference's first maximiser, before any backward"""
    b8, heavy_of, arg_h = state.decode(label)
    n, H = S.n, state.H
    deg = S.deg
    heavy = deg > S.chunk
    light = (deg > 0) & ~heavy
    assert bool((b8[light] < deg[light].view(-1, 1)).all()), \
        f"{label}: a light row holds an offset >= its degree (the backward would take it for another edge or a heavy row)"
    assert bool((b8[deg == 0] == 0).all()), f"{label}: an empty row's state is not 0"
    hr = heavy.nonzero().flatten()
    assert bool((b8[heavy] == 255).all()), f"{label}: a heavy row lacks the marker in some column"
    assert torch.equal(heavy_of[hr], torch.arange(hr.numel())), f"{label}: heavy_of of the heavy rows"
    assert bool((arg_h >= 0).all()) and bool((arg_h < deg[hr].view(-1, 1)).all()), f"{label}: arg_h outside [0, deg)"
    off = b8.clone()
    off[hr] = arg_h
    assert torch.equal(off, ref["off"]), \
        f"{label}: {int((off != ref['off']).sum())} offsets differ from the first maximiser in CSR order"
    if S.E:
        pos = (S.rowptr[:-1].view(-1, 1) + off).clamp_max(S.E - 1)
        at = x[S.col[pos], torch.arange(H).view(1, -1).expand(n, -1)]
        w = ref["winner"]
        assert torch.equal(at[w].view(torch.int32), out[w].view(torch.int32)), f"{label}: x at the argmax is not the output"
        none = (deg > 0).view(-1, 1) & ~w
        assert bool((out[none] == R.NEG_INF).all()) and bool((off[none] == 0).all()), \
            f"{label}: a column without a winner must give -inf and offset 0"


def run_fwd(dev, G, x, hv, reduce, state=None):
    H = hv[0]
    csr = G["fwd"]
    xin, ldo = windows(dev, x, hv)
    out, part = Out(dev, G["n"], H, ld=ldo), scratch_for(dev, csr, H, 2 if reduce == MAX else 1)
    _lib.call("bgnn_spmm_fwd", csr.ref(), ptr(xin), xin.ld, H, reduce, ptr(out), out.ld, ptr(state),
              ptr(part) if csr.plan.n_chunks else None, _stream())
    torch.cuda.synchronize()
    out.guard("bgnn_spmm_fwd out")
    part.guard("bgnn_spmm_fwd chunk scratch")
    return out.read()


def run_bwd(dev, G, g, hv, reduce, addend=None, amax=None, state=None, csr=None, heavy_done=0, init=None):
    """the three transposes: state given = bgnn_spmm_bwd_max, addend given = bgnn_spmm_bwd_add"""
    H = hv[0]
    csr = G["bwd"] if csr is None else csr
    gin, ldo = windows(dev, g, hv)
    ain = None if addend is None else In(dev, addend)
    gx, part = Out(dev, G["n"], H, ld=ldo, init=init), scratch_for(dev, csr, H)
    pp = ptr(part) if csr.plan.n_chunks else None
    pt, frp = G["perm_t"].data_ptr(), G["frp"].data_ptr()
    if state is not None:
        _lib.call("bgnn_spmm_bwd_max", csr.ref(), pt, frp, G["n"], ptr(gin), gin.ld, H, ptr(state), ptr(ain),
                  ain.ld if ain else 0, ptr(gx), gx.ld, pp, ptr(amax), _stream())
    elif addend is not None:
        _lib.call("bgnn_spmm_bwd_add", csr.ref(), None, frp, ptr(gin), gin.ld, H, reduce, ptr(ain), ain.ld, ptr(gx),
                  gx.ld, pp, ptr(amax), _stream())
    else:   # SUM needs neither perm_t nor the forward rowptr
        _lib.call("bgnn_spmm_bwd", csr.ref(), None, frp if reduce == MEAN else None, ptr(gin), gin.ld, H, reduce, ptr(gx),
                  gx.ld, pp, ptr(amax), heavy_done, _stream())
    torch.cuda.synchronize()
    gx.guard("transpose gx")
    part.guard("transpose chunk scratch")
    return gx.read()


def hv_id(hv):
    return f"{hv[0]}{hv[1]}"


OTHERS = ("hand_r8", "hand_nogroups", "store", "hand_t") + R.CHUNKED + R.TINY
CASES = [("hand", hv) for hv in R.H_CASES] + [(k, hv) for k in OTHERS for hv in R.H_SHORT]
IDS = [f"{k}-{hv_id(hv)}" for k, hv in CASES]


# ============================================================================ A. bgnn_spmm_fwd SUM / MEAN
@pytest.mark.parametrize("kind,hv", CASES, ids=IDS)
def test_a_fwd_sum_mean(dev, kind, hv):
    G = dev_graph(kind, dev)
    x = R.randn_rows(kind, hv[0], 0)
    for reduce in (SUM, MEAN):
        ref, bound = R.fwd_ref(kind, x, reduce)
        label = f"bgnn_spmm_fwd {kind} N={G['n']} H={hv_id(hv)} {'mean' if reduce else 'sum'}"
        res = []
        for cfg in configs(kind, hv, kind == "hand"):
            set_knobs(**cfg)
            fam = family_of(G, G["fwd"], hv, cfg, True)
            o = run_fwd(dev, G, x, hv, reduce)
            check(f"spmm A fwd {'mean' if reduce else 'sum'} ({fam})", o, ref, bound, f"{label} {fam} {cfg}")
            assert bool((o[G["S"].deg == 0] == 0).all()), f"{label}: an empty row is not 0"
            res.append((fam, cfg, o))
        exact_claims(res, G, G["fwd"], label)
        set_knobs(**res[0][1])
        assert torch.equal(run_fwd(dev, G, x, hv, reduce).view(torch.int32), res[0][2].view(torch.int32)), \
            f"{label}: two runs differ"


# ============================================================================ B. MAX forward, state, backward
def max_cases():
    """hand: the ties and the non-finite inputs at every H, randn at one H per family; the other
    structures with heavy rows or a chunk of their own (store, chunk 200 -- bgnn_spmm_fwd(arg) takes a
    chunk below 255, and its light rows then reach offsets above 64 --, tiny5): ties and non-finite
    inputs at one H per family; the rest: ties at a scalar, a row-per-wave and a tiled H"""
    out = [("hand", hv, s) for s in ("ties", "nonfinite") for hv in R.H_CASES]
    out += [("hand", hv, "randn") for hv in R.H_SHORT]
    out += [(k, hv, s) for k in ("store", "hand_c200", "tiny5") for s in ("ties", "nonfinite") for hv in R.H_SHORT]
    out += [(k, hv, "ties") for k in OTHERS if k not in ("store", "hand_c200", "tiny5") for hv in R.H_SHORT[::2]]
    return out


MAX_CASES = max_cases()


def max_input(kind, H, which):
    return {"randn": lambda: R.randn_rows(kind, H, 0), "ties": lambda: R.ties_rows(kind, H),
            "nonfinite": lambda: R.nonfinite_rows(kind, H)}[which]()


def max_forward_and_state(dev, G, x, hv, ref, label, cfgs):
    """every configuration: the value exact with arg NULL and non-NULL, the state checked on the host.
    -> the last checked state"""
    S = G["S"]
    want = ref["out"].float()
    state = None
    for cfg in cfgs:
        set_knobs(**cfg)
        fam = family_of(G, G["fwd"], hv, cfg, False)
        o = run_fwd(dev, G, x, hv, MAX)
        assert torch.equal(o.view(torch.int32), want.view(torch.int32)), \
            f"{label} {fam} {cfg} arg=NULL: {int((o.view(torch.int32) != want.view(torch.int32)).sum())} values differ"
        state = ArgState(dev, S.n, hv[0], G["fwd"].plan.n_heavy)
        o2 = run_fwd(dev, G, x, hv, MAX, state)
        assert torch.equal(o2.view(torch.int32), want.view(torch.int32)), f"{label} {fam} {cfg} with arg: values differ"
        check_state(state, S, G["fwd"], x, o2, ref, f"{label} {fam} {cfg}")
    return state


def max_backward(dev, G, kind, x, hv, state, label, i, fwd):
    """bgnn_spmm_bwd_max on a state that passed check_state, without and with an addend"""
    H = hv[0]
    g, a = R.randn_rows(kind, H, 1), R.randn_rows(kind, H, 2)
    for addend in (None, a):
        ref, bound = R.max_bwd_ref(kind, x, g, addend, fwd=fwd)
        res = []
        for j, cfg in enumerate(configs(kind, hv, False)):
            set_knobs(**cfg)
            fam = family_of(G, G["bwd"], hv, cfg, False)
            prev = amax_prev(i + j)
            am = scalar(dev, prev) if j != 1 else None
            o = run_bwd(dev, G, g, hv, MAX, addend, am, state)
            lab = f"{label} bwd_max addend={'given' if addend is not None else 'NULL'} {fam} {cfg}"
            check(f"spmm B bwd_max{' + addend' if addend is not None else ''}", o, ref, bound, lab)
            if am is not None:
                check_amax(am, prev, o, lab)
            res.append((fam, cfg, o))
        exact_claims(res, G, G["bwd"], label + " bwd_max")


@pytest.mark.parametrize("i", range(len(MAX_CASES)), ids=[f"{k}-{hv_id(hv)}-{s}" for k, hv, s in MAX_CASES])
def test_b_max(dev, i):
    kind, hv, which = MAX_CASES[i]
    G = dev_graph(kind, dev)
    x = max_input(kind, hv[0], which)
    ref = R.max_fwd_ref(kind, x)
    label = f"bgnn_spmm_fwd {kind} N={G['n']} H={hv_id(hv)} max, {which} inputs"
    cfgs = configs(kind, hv, kind == "hand" and which == "ties")
    state = max_forward_and_state(dev, G, x, hv, ref, label, cfgs)
    max_backward(dev, G, kind, x, hv, state, label, i, ref)
    set_knobs(**cfgs[0])
    again = ArgState(dev, G["n"], hv[0], G["fwd"].plan.n_heavy)
    run_fwd(dev, G, x, hv, MAX, again)
    first = ArgState(dev, G["n"], hv[0], G["fwd"].plan.n_heavy)
    run_fwd(dev, G, x, hv, MAX, first)
    for p, q in zip(again.decode(label), first.decode(label)):
        assert torch.equal(p, q), f"{label}: the state differs between two runs"


# ============================================================================ C. the transposes
@pytest.mark.parametrize("i", range(len(CASES)), ids=IDS)
def test_c_bwd_sum_mean(dev, i):
    kind, hv = CASES[i]
    G = dev_graph(kind, dev)
    H = hv[0]
    g, a = R.randn_rows(kind, H, 1), R.randn_rows(kind, H, 2)
    for reduce in (SUM, MEAN):
        for addend in (None, a):
            ref, bound = R.bwd_ref(kind, g, reduce, addend)
            name = "bgnn_spmm_bwd_add" if addend is not None else "bgnn_spmm_bwd"
            label = f"{name} {kind} N={G['n']} H={hv_id(hv)} {'mean' if reduce else 'sum'}"
            res = []
            for j, cfg in enumerate(configs(kind, hv, kind == "hand" and addend is None)):
                set_knobs(**cfg)
                fam = family_of(G, G["bwd"], hv, cfg, True)
                prev = amax_prev(i + j)
                am = scalar(dev, prev) if j != 1 else None        # the second configuration: amax NULL
                o = run_bwd(dev, G, g, hv, reduce, addend, am)
                check(f"spmm C {name[5:]} {'mean' if reduce else 'sum'} ({fam})", o, ref, bound, f"{label} {fam} {cfg}")
                if am is not None:
                    check_amax(am, prev, o, f"{label} {fam} {cfg}")
                res.append((fam, cfg, o))
            exact_claims(res, G, G["bwd"], label)
    set_knobs(**res[0][1])
    assert torch.equal(run_bwd(dev, G, g, hv, MEAN, a).view(torch.int32), res[0][2].view(torch.int32)), \
        f"{label}: two runs differ"


# ============================================================================ D. heavy_done
_ranged = {}


@pytest.mark.parametrize("reduce", [SUM, MEAN])
@pytest.mark.parametrize("hv", R.H_SHORT + [(100, "off4")], ids=hv_id)
def test_d_bwd_heavy_done(dev, hv, reduce):
    """bgnn_spmm_bwd with heavy_done = 1 on the store batch: the range rows' gx rows keep what they
    held, every other row meets the bound, amax ignores the skipped rows"""
    G = dev_graph("store", dev)
    if "t" not in _ranged:
        s = G["bwd"]
        c = Csr(s.rowptr, s.col, s.n_rows, s.nnz, s.plan, s.groups)   # a copy: ranges stay off the shared one
        c.ensure_ranges()
        assert c.ranges_all == 1
        _ranged["t"] = c
    csr = _ranged["t"]
    H, n = hv[0], G["n"]
    rg = csr.ranges.cpu()
    nh = csr.plan.n_heavy
    heavy = csr.plan.heavy_row[:nh].cpu().long()
    assert int(rg[0]) == nh == 3
    skipped = torch.zeros(n, dtype=torch.bool)
    skipped[heavy[rg[4:2 + 3 * nh:3].long()]] = True
    assert int(skipped.sum()) == 3 and torch.equal(skipped, G["S"].deg_t > 64)
    g = R.randn_rows("store", H, 1)
    ref, bound = R.bwd_ref("store", g, reduce)
    init = torch.full((n, H), float("nan"))
    init[skipped] = 12345.0 + torch.arange(H)          # above every |gx|: amax must not see it
    label = f"bgnn_spmm_bwd store N={n} H={hv_id(hv)} {'mean' if reduce else 'sum'} heavy_done=1"
    res = []
    for cfg in configs("store", hv, False):
        set_knobs(**cfg)
        fam = family_of(G, csr, hv, cfg, True)
        am = scalar(dev, 0.0)
        o = run_bwd(dev, G, g, hv, reduce, None, am, csr=csr, heavy_done=1, init=init)
        assert torch.equal(o[skipped].view(torch.int32), init[skipped].view(torch.int32)), \
            f"{label} {fam}: a range row's gx row was written"
        check(f"spmm D heavy_done ({fam})", o[~skipped], ref[~skipped], bound[~skipped], f"{label} {fam} {cfg}")
        check_amax(am, 0.0, o[~skipped], f"{label} {fam} {cfg}")
        res.append((fam, cfg, torch.where(skipped.view(-1, 1), torch.zeros(()), o)))
    exact_claims(res, G, csr, label)
    full = run_bwd(dev, G, g, hv, reduce, None, None, csr=csr, heavy_done=0)   # the same CSR without the skip
    check(f"spmm D heavy_done ({res[0][0]})", full, ref, bound, label + " (heavy_done=0 on the ranged CSR)")


# ============================================================================ E. bgnn_spmm_max_bf16's state
@pytest.mark.parametrize("which", ["ties", "nonfinite"])
@pytest.mark.parametrize("H", [64, 512])
def test_e_bf16_state(dev, H, which):
    kind = "hand"
    G = dev_graph(kind, dev)
    S, csr, n = G["S"], G["fwd"], G["n"]
    xb = max_input(kind, H, which).bfloat16()
    x = xb.float()
    ref = R.max_fwd_ref(kind, x)
    label = f"bgnn_spmm_max_bf16 {kind} N={n} H={H} {which} inputs"
    xd = torch.cat([xb, torch.full((2, H), float("nan"), dtype=torch.bfloat16)]).to(dev)
    states = []
    for _ in range(2):
        out = torch.full((n + 2, H), float("nan"), dtype=torch.bfloat16, device=dev)
        state, part = ArgState(dev, n, H, csr.plan.n_heavy), scratch_for(dev, csr, H, 2)
        _lib.call("bgnn_spmm_max_bf16", csr.ref(), xd.data_ptr(), H, H, out.data_ptr(), H, ptr(state), ptr(part), _stream())
        torch.cuda.synchronize()
        part.guard(label + " chunk scratch")
        o = out.cpu().float()
        assert bool(torch.isnan(o[n:]).all()), f"{label}: a row after the last one was written"
        assert torch.equal(o[:n].view(torch.int32), ref["out"].float().view(torch.int32)), f"{label}: values differ"
        check_state(state, S, csr, x, o[:n], ref, label)
        states.append(state)
    for p, q in zip(states[0].decode(label), states[1].decode(label)):
        assert torch.equal(p, q), f"{label}: the state differs between two runs"
    max_backward(dev, G, kind, x, (H, ""), states[0], label, H, ref)


# ============================================================================ F. no rows
def test_f_no_rows(dev):
    """N = 0: BGNN_OK, nothing written"""
    z = torch.zeros(2, dtype=torch.int32, device=dev)
    csr = Csr(z[:1], z[:1], 0, 0, Plan(z[:1], z, z[:1], 0, 0, 64))
    x = In(dev, torch.zeros(0, 8))
    for reduce in (SUM, MEAN, MAX):
        out = Out(dev, 0, 8)
        _lib.call("bgnn_spmm_fwd", csr.ref(), ptr(x), x.ld, 8, reduce, ptr(out), out.ld, None, None, _stream())
        am = scalar(dev, 0.25)
        if reduce != MAX:
            _lib.call("bgnn_spmm_bwd", csr.ref(), None, z.data_ptr(), ptr(x), x.ld, 8, reduce, ptr(out), out.ld, None,
                      ptr(am), 0, _stream())
            _lib.call("bgnn_spmm_bwd_add", csr.ref(), None, z.data_ptr(), ptr(x), x.ld, 8, reduce, ptr(x), x.ld, ptr(out),
                      out.ld, None, ptr(am), _stream())
        else:
            state = ArgState(dev, 0, 8, 0)
            _lib.call("bgnn_spmm_bwd_max", csr.ref(), z.data_ptr(), z.data_ptr(), 0, ptr(x), x.ld, 8, ptr(state), None, 0,
                      ptr(out), out.ld, None, ptr(am), _stream())
            state.decode("N = 0")
        torch.cuda.synchronize()
        out.guard("N = 0")
        assert am.read().item() == 0.25
