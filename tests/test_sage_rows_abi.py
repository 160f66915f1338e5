"""C-ABI of the f32 SAGE layer row kernels (csrc/sage.hip) and of bgnn_sage_fwd: every argument
check answers BGNN_E_ARG with its message before anything touches a device (no GPU here: the
pointers below are never dereferenced, and every call in this file is one the library rejects
before a launch -- or, for n_rows == 0 of bgnn_sage_apply, returns before one)."""
import ctypes

import pytest

P = 4096   # a 16-byte aligned non-NULL "pointer"
Q = P + 4  # a misaligned one


_CSRS = {"no_rowptr": dict(rowptr=None), "heavy": dict(n_chunks=3, n_heavy=1), "ranges": dict(ranges=P)}


def _csr(**kw):
    from bgnn import _lib

    f = dict(rowptr=P, col=P, heavy_row=P, heavy_chunk0=P, chunk_heavy=P, n_rows=100, nnz=800, n_heavy=0,
             n_chunks=0, chunk=64)
    f.update(kw)
    return _lib.CsrStruct(**f)


def apply_(o=P, scale=P, shift=P, x_prev=P, skip=1, p=0.1, seed=7, n_rows=10, H=64, x_next=P, amax=P, ranges=None,
           range_partial=None):
    return ("bgnn_sage_apply", o, scale, shift, x_prev, skip, p, seed, n_rows, H, x_next, amax, ranges, range_partial,
            None)


def stats(g=P, g_rows=None, o=P, scale=P, shift=P, mean=P, invstd=P, p=0.1, seed=7, n_rows=10, H=64, partial2=P):
    return ("bgnn_sage_bwd_stats", g, g_rows, o, scale, shift, mean, invstd, p, seed, n_rows, H, partial2, None)


def rows(g=P, g_rows=None, o=P, nrm=P, scale=P, shift=P, gamma=P, mean=P, invstd=P, sum_g2=P, sum_g2xhat=P, p=0.1,
         seed=7, skip=1, n_rows=10, H=64, dh=P, lddh=64, gskip=P, partial_db=P, amax=P, w_rowptr=None, w_mode=0,
         ranges=None, range_w_rowptr=None, range_partial=None):
    return ("bgnn_sage_bwd_rows", g, g_rows, o, nrm, scale, shift, gamma, mean, invstd, sum_g2, sum_g2xhat, p, seed,
            skip, n_rows, H, dh, lddh, gskip, partial_db, amax, w_rowptr, w_mode, ranges, range_w_rowptr,
            range_partial, None)


def l2(g=P, o=P, nrm=P, n_rows=10, H=64, dh=P, lddh=64, partial_db=P, amax=P):
    return ("bgnn_l2norm_bwd", g, o, nrm, n_rows, H, dh, lddh, partial_db, amax, None)


def fwd(csr=None, zl=P, ldzl=128, zr=P + 256, ldzr=128, bias=P, H=64, reduce=0, o=P, nrm=P, bn_partial=P,
        partial=None, heavy_agg=None, ld_heavy_agg=0, null_csr=False):
    c = _csr(**_CSRS[csr]) if csr else _csr()   # (byref keeps the struct alive)
    return ("bgnn_sage_fwd", None if null_csr else ctypes.byref(c), zl, ldzl, zr, ldzr, bias, H, reduce, o, nrm,
            bn_partial, partial, heavy_agg, ld_heavy_agg, None)


def prep(g=P, y=P, N=10, C=64, g_out=P, partial=P, amax=P):
    return ("bgnn_linear_bwd_prep", g, y, N, C, g_out, partial, amax, None)


def prep16(g=P, y=P, N=10, C=64, g_out=P, partial=P):
    return ("bgnn_linear_bwd_prep_bf16", g, y, N, C, g_out, partial, None)


def reduce_(partial=P, n_slots=4, H=64, out0=P, out1=P, acc=0):
    return ("bgnn_reduce_partials", partial, n_slots, H, out0, out1, acc, None)


def fin(part=P, n_slots=4, H=64, count=10, mean=P, invstd=P, scale=P, shift=P):
    return ("bgnn_bn_finalize", part, n_slots, H, count, P, P, 1e-5, 0.1, P, P, mean, invstd, scale, shift, None)


def fin_s(part=P, n_slots=4, H=64, count=10, kshift=P, mean=P, invstd=P, scale=P, shift=P):
    return ("bgnn_bn_finalize_shifted", part, n_slots, H, count, kshift, P, P, 1e-5, 0.1, P, P, mean, invstd, scale,
            shift, None)


def evalc(H=64, rmean=P, rvar=P, scale=P, shift=P):
    return ("bgnn_bn_eval_coeffs", H, P, P, 1e-5, rmean, rvar, scale, shift, None)


CHECKS = [
    # ---- bgnn_sage_apply
    (apply_(o=None), "sage_apply: null o / x_next"),
    (apply_(x_next=None), "sage_apply: null o / x_next"),
    (apply_(n_rows=-1), "sage_apply: negative n_rows"),
    (apply_(H=66), "sage_apply: H must be a multiple of 4"),
    (apply_(H=0), "sage_apply: H must be a multiple of 4"),
    (apply_(p=1.0), "dropout p must be in \\[0, 1\\)"),
    (apply_(p=-0.5), "dropout p must be in \\[0, 1\\)"),
    (apply_(p=float("nan")), "dropout p must be in \\[0, 1\\)"),
    (apply_(scale=None), "scale/shift must both be set or NULL"),
    (apply_(shift=None), "scale/shift must both be set or NULL"),
    (apply_(x_prev=None), "skip requires x_prev"),
    (apply_(o=Q), "sage_apply: pointers must be 16-byte aligned"),
    (apply_(x_next=Q), "sage_apply: pointers must be 16-byte aligned"),
    (apply_(x_prev=Q, skip=0), "sage_apply: pointers must be 16-byte aligned"),
    (apply_(scale=Q), "sage_apply: pointers must be 16-byte aligned"),
    (apply_(shift=Q), "sage_apply: pointers must be 16-byte aligned"),
    (apply_(ranges=P), "ranges need a 16-B aligned range_partial and H <= 512"),
    (apply_(ranges=P, range_partial=Q), "ranges need a 16-B aligned range_partial and H <= 512"),
    (apply_(ranges=P, range_partial=P, H=516), "ranges need a 16-B aligned range_partial and H <= 512"),
    # ---- bgnn_sage_bwd_stats
    (stats(n_rows=-1), "sage_bwd_stats: negative n_rows"),
    (stats(H=66), "sage_bwd_stats: H=66 unsupported"),
    (stats(H=1028), "sage_bwd_stats: H=1028 unsupported"),
    (stats(H=0), "sage_bwd_stats: H=0 unsupported"),
] + [(stats(**{k: None}), "sage_bwd_stats: null pointer")
     for k in ("g", "o", "scale", "shift", "mean", "invstd", "partial2")] + [
    (stats(**{k: Q}), "sage_bwd_stats: pointers must be 16-byte aligned")
    for k in ("g", "o", "scale", "shift", "mean", "invstd", "partial2")] + [
    # ---- bgnn_sage_bwd_rows
    (rows(n_rows=-1), "sage_bwd_rows: negative n_rows"),
] + [(rows(**{k: None}), "sage_bwd_rows: null pointer") for k in ("g", "o", "nrm", "dh", "partial_db")] + [
    (rows(H=66, lddh=68), "sage_bwd_rows: H=66 unsupported"),
    (rows(H=516, lddh=516), "sage_bwd_rows: H=516 unsupported"),
    (rows(H=0), "sage_bwd_rows: H=0 unsupported"),
    (rows(w_mode=1), "sage_bwd_rows: bad row weights"),
    (rows(w_mode=2), "sage_bwd_rows: bad row weights"),
    (rows(w_mode=3, w_rowptr=P), "sage_bwd_rows: bad row weights"),
    (rows(w_mode=-1, w_rowptr=P), "sage_bwd_rows: bad row weights"),
    (rows(lddh=60), "sage_bwd_rows: bad lddh"),
    (rows(lddh=66), "sage_bwd_rows: bad lddh"),
    (rows(gskip=None), "sage_bwd_rows: skip requires gskip"),
    (rows(invstd=None), "sage_bwd_rows: BN stats incomplete"),
    (rows(sum_g2=None), "sage_bwd_rows: BN stats incomplete"),
    (rows(sum_g2xhat=None), "sage_bwd_rows: BN stats incomplete"),
] + [(rows(**{k: Q}), "sage_bwd_rows: pointers must be 16-byte aligned")
     for k in ("g", "o", "dh", "gskip", "partial_db")] + [
    (rows(ranges=P), "sage_bwd_rows: ranges need range_partial"),
    (rows(ranges=P, range_partial=Q), "sage_bwd_rows: ranges need range_partial"),
    # ---- bgnn_l2norm_bwd
    (l2(n_rows=-1), "l2norm_bwd: negative n_rows"),
    (l2(H=66, lddh=68), "l2norm_bwd: H=66 unsupported"),
    (l2(H=516, lddh=516), "l2norm_bwd: H=516 unsupported"),
] + [(l2(**{k: None}), "l2norm_bwd: null pointer") for k in ("g", "o", "nrm", "dh", "partial_db", "amax")] + [
    (l2(lddh=60), "l2norm_bwd: bad lddh"),
    (l2(lddh=66), "l2norm_bwd: bad lddh"),
] + [(l2(**{k: Q}), "l2norm_bwd: pointers must be 16-byte aligned") for k in ("g", "o", "dh", "partial_db")] + [
    # ---- bgnn_linear_bwd_prep (f32 and bf16)
    (prep(g=None), "linear_bwd_prep: null pointer or negative size"),
    (prep(partial=None), "linear_bwd_prep: null pointer or negative size"),
    (prep(amax=None), "linear_bwd_prep: null pointer or negative size"),
    (prep(N=-1), "linear_bwd_prep: null pointer or negative size"),
    (prep(g_out=None), "linear_bwd_prep: a ReLU mask needs g_out"),
    (prep(C=12), "linear_bwd_prep: C = 12 must be 4 \\* a power of two"),
    (prep(C=2048), "linear_bwd_prep: C = 2048 must be 4 \\* a power of two"),
    (prep(C=0), "linear_bwd_prep: C = 0 must be"),
    (prep(g=Q), "linear_bwd_prep: pointers must be 16-B aligned"),
    (prep(y=Q), "linear_bwd_prep: pointers must be 16-B aligned"),
    (prep(g_out=Q), "linear_bwd_prep: pointers must be 16-B aligned"),
    (prep(partial=Q), "linear_bwd_prep: pointers must be 16-B aligned"),
    (prep16(g=None), "linear_bwd_prep_bf16: null pointer or negative size"),
    (prep16(g_out=None), "linear_bwd_prep_bf16: a ReLU mask needs g_out"),
    (prep16(C=4), "linear_bwd_prep_bf16: C = 4 must be 8 \\* a power of two"),
    (prep16(C=24), "linear_bwd_prep_bf16: C = 24 must be 8 \\* a power of two"),
    (prep16(partial=Q), "linear_bwd_prep_bf16: pointers must be 16-B aligned"),
    # ---- reductions and BatchNorm coefficients
    (reduce_(partial=None), "reduce_partials: bad args"),
    (reduce_(H=0), "reduce_partials: bad args"),
    (reduce_(n_slots=-1), "reduce_partials: bad args"),
    (fin(part=None), "bn_finalize: bad args"),
    (fin(H=0), "bn_finalize: bad args"),
    (fin(count=0), "bn_finalize: bad args"),
] + [(fin(**{k: None}), "bn_finalize: bad args") for k in ("mean", "invstd", "scale", "shift")] + [
    (fin_s(part=None), "bn_finalize_shifted: bad args"),
    (fin_s(kshift=None), "bn_finalize_shifted: bad args"),
    (fin_s(count=0), "bn_finalize_shifted: bad args"),
    (fin_s(shift=None), "bn_finalize_shifted: bad args"),
    (evalc(H=0), "bn_eval_coeffs: bad args"),
] + [(evalc(**{k: None}), "bn_eval_coeffs: bad args") for k in ("rmean", "rvar", "scale", "shift")] + [
    # ---- bgnn_sage_fwd
    (fwd(null_csr=True), "sage_fwd: null csr"),
    (fwd(csr="no_rowptr"), "sage_fwd: null csr"),
    (fwd(H=66, ldzl=132, ldzr=132), "sage_fwd: H=66 unsupported"),
    (fwd(H=516, ldzl=1032, ldzr=1032), "sage_fwd: H=516 unsupported"),
    (fwd(H=0), "sage_fwd: H=0 unsupported"),
    (fwd(ldzl=60), "ldzl/ldzr must be >= H and multiples of 4"),
    (fwd(ldzl=66), "ldzl/ldzr must be >= H and multiples of 4"),
    (fwd(ldzr=60), "ldzl/ldzr must be >= H and multiples of 4"),
    (fwd(ldzr=66), "ldzl/ldzr must be >= H and multiples of 4"),
    (fwd(reduce=2), "sage_fwd: reduce must be sum/mean"),
    (fwd(reduce=-1), "sage_fwd: reduce must be sum/mean"),
] + [(fwd(**{k: Q}), "sage_fwd: pointers must be 16-byte aligned") for k in ("zl", "zr", "o", "bias", "bn_partial")] + [
    (fwd(csr="heavy", partial=Q), "sage_fwd: pointers must be 16-byte aligned"),
    (fwd(csr="heavy"), "sage_fwd: partial scratch required for heavy rows"),
    (fwd(heavy_agg=P, ld_heavy_agg=64), "heavy_agg needs the CSR's ranges"),
    (fwd(csr="ranges", heavy_agg=Q, ld_heavy_agg=64), "heavy_agg needs the CSR's ranges, 16-B alignment"),
    (fwd(csr="ranges", heavy_agg=P, ld_heavy_agg=60), "heavy_agg needs the CSR's ranges, 16-B alignment and ld >= H"),
    (fwd(csr="ranges", heavy_agg=P, ld_heavy_agg=66), "heavy_agg needs the CSR's ranges, 16-B alignment and ld >= H"),
]

@pytest.mark.parametrize("i", range(len(CHECKS)), ids=[f"{c[0][0][5:]}-{i}" for i, c in enumerate(CHECKS)])
def test_argument_checks(i):
    from bgnn import _lib

    args, msg = CHECKS[i]
    name, args = args[0], args[1:]
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _lib.call(name, *args)
    assert e.value.code == 1001, f"{name}: {e.value}"   # BGNN_E_ARG; a HIP code means the call reached a launch


def test_sage_apply_without_rows_is_a_no_op():
    """n_rows == 0 returns before any launch, also with NULL o / x_next."""
    from bgnn import _lib

    name, *args = apply_(n_rows=0, o=None, x_next=None)
    assert _lib.call(name, *args) == 0
