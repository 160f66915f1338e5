"""C-ABI of bgnn_readout_index (additive at ABI 22): the header declares it, the library exports it,
the Python binding agrees on the argument count, and every argument check answers BGNN_E_ARG with
its message before anything touches a device (no GPU here: the pointers below are never
dereferenced, and every call in this file is one the library rejects before a launch)."""
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "bgnn.h")
P = 4096   # a non-NULL "pointer"
NAME = "bgnn_readout_index"


def test_header_library_and_binding_agree():
    from bgnn import _lib

    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    assert int(re.search(r"#define\s+BGNN_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION >= 22
    lib = _lib.load()
    assert lib.bgnn_abi_version() == _lib.ABI_VERSION
    decl = re.search(r"\b" + NAME + r"\s*\(([^)]*)\)", text)
    assert decl and hasattr(lib, NAME)
    assert len(_lib.SIGNATURES[NAME][1]) == len(decl.group(1).split(",")) == 11


def index_(ptr=P, B=3, N=100, min_nodes=2, max_nodes=50, rowptr2=P, seg_of_row=P, real_index=P, real_batch=P,
           real_rowptr=P):
    return (NAME, ptr, B, N, min_nodes, max_nodes, rowptr2, seg_of_row, real_index, real_batch, real_rowptr, None)


CHECKS = [
    (index_(B=0), "readout_index: batch of 0 graphs unsupported"),
    (index_(B=-1), "readout_index: batch of -1 graphs unsupported"),
    (index_(B=65536, N=1 << 20), "readout_index: batch of 65536 graphs unsupported"),
    (index_(N=2), "readout_index: N 2 out of range for 3 graphs"),
    (index_(N=1 << 31), "readout_index: N 2147483648 out of range"),
    (index_(min_nodes=0), "a graph with fewer than 1 node has no super node"),
    (index_(min_nodes=-4), "a graph with fewer than 1 node has no super node"),
    (index_(max_nodes=1), "readout_index: max_nodes 1 out of range"),
    (index_(max_nodes=101), "readout_index: max_nodes 101 out of range"),
    (index_(ptr=None), "readout_index: null pointer"),
    (index_(rowptr2=None), "readout_index: null pointer"),
    (index_(seg_of_row=None), "readout_index: null pointer"),
    (index_(real_rowptr=None), "readout_index: null pointer"),
    (index_(real_index=None), "readout_index: null real-node arrays"),
    (index_(real_batch=None), "readout_index: null real-node arrays"),
]


@pytest.mark.parametrize("i", range(len(CHECKS)), ids=[str(i) for i in range(len(CHECKS))])
def test_argument_checks(i):
    from bgnn import _lib

    args, msg = CHECKS[i]
    with pytest.raises(_lib.BgnnError, match=msg) as e:
        _lib.call(args[0], *args[1:])
    assert e.value.code == 1001, str(e.value)   # BGNN_E_ARG; a HIP code means the call reached a launch


def test_stale_argument_count_is_refused():
    from bgnn import _lib

    name, *args = index_()
    with pytest.raises(TypeError, match="takes 11 arguments"):
        _lib.call(name, *args[:-1])

