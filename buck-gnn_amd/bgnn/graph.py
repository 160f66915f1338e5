"""Device-side graph structure: edge_index -> CSR (+ transpose) and heavy-row plans.

PyG's `SAGEConv(x, edge_index)` (flow='source_to_target') aggregates, for every
target i = edge_index[1, e], the source rows j = edge_index[0, e]
(Models/BuckGNN.py:342,434). Here edge_index is sorted once per distinct tensor
into a CSR over targets (for the forward) and a CSR over sources (for the
backward), both stable, by `bgnn_graph_build`. Rows with more than `chunk`
entries (the super node of VirtualEdgeCreate.py:81-113 has in-degree N_g) get a
split plan so that one wave never walks thousands of neighbours alone.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass, field
from typing import Optional

import numpy as np
import torch

from . import _lib

DEFAULT_CHUNK = 64
# Rows per row-group of the sum/mean aggregation kernels (bgnn_group_plan; 0 = no plans, the
# per-row sweep kernel). Consecutive mesh rows share most neighbours: with 4 rows per group cfg2
# fetches 5.5 source rows per target row instead of 8.9 (8 rows: 4.7, but twice the registers
# and half the waves per CU; measured slower, tools/tune_agg.py).
GROUP_ROWS = 4


def _ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else t.data_ptr()


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


def require_cuda(*tensors: torch.Tensor, what: str = "bgnn") -> None:
    for t in tensors:
        if t is not None and not t.is_cuda:
            raise RuntimeError(
                f"{what}: tensors must be on a ROCm GPU (got device {t.device}); "
                "bgnn has no CPU fallback")


@dataclass
class Plan:
    """Heavy-row split plan of one CSR (rows with deg > chunk). n_heavy / n_chunks are
    filled on the host after the (single, batched) device->host copy of the counts."""

    heavy_row: torch.Tensor
    heavy_chunk0: torch.Tensor
    chunk_heavy: torch.Tensor
    n_heavy: int
    n_chunks: int
    chunk: int


def enqueue_plan(rowptr: torch.Tensor, n_rows: int, nnz: int, counts: torch.Tensor,
                 chunk: int = DEFAULT_CHUNK) -> Plan:
    """Launch bgnn_heavy_plan; its two counts land in `counts` (device int32[2])."""
    dev = rowptr.device
    heavy_row = torch.empty(max(n_rows, 1), dtype=torch.int32, device=dev)
    heavy_chunk0 = torch.empty(max(n_rows, 1) + 1, dtype=torch.int32, device=dev)
    # sum over heavy rows of ceil(deg/chunk) <= nnz/chunk + n_heavy <= 2*nnz/chunk
    chunk_heavy = torch.empty(2 * (nnz // chunk) + 2, dtype=torch.int32, device=dev)
    ws = torch.empty(_lib.query("bgnn_heavy_plan_ws_bytes", n_rows), dtype=torch.uint8, device=dev)
    _lib.call("bgnn_heavy_plan", rowptr.data_ptr(), n_rows, nnz, chunk, heavy_row.data_ptr(),
              heavy_chunk0.data_ptr(), chunk_heavy.data_ptr(), counts.data_ptr(), ws.data_ptr(), ws.numel(),
              _stream())
    return Plan(heavy_row, heavy_chunk0, chunk_heavy, -1, -1, chunk)


def make_plan(rowptr: torch.Tensor, n_rows: int, nnz: int, chunk: int = DEFAULT_CHUNK) -> Plan:
    counts = torch.empty(2, dtype=torch.int32, device=rowptr.device)
    p = enqueue_plan(rowptr, n_rows, nnz, counts, chunk)
    p.n_heavy, p.n_chunks = counts.tolist()
    return p


@dataclass
class Groups:
    """Row-group plan of a CSR (bgnn_group_plan): per group of at most `rows` consecutive rows,
    its distinct source rows (gsrc) and the mask of the group rows using each (gmask). `grow`
    (optional, [n_groups + 1]) holds each group's first row; None means g * rows."""

    gsrc: torch.Tensor
    gmask: torch.Tensor
    gcnt: torch.Tensor
    rows: int
    grow: Optional[torch.Tensor] = None
    n_groups: int = 0


def enqueue_groups(rowptr: torch.Tensor, col: torch.Tensor, n_rows: int, nnz: int, chunk: int,
                   rows: Optional[int] = None, grow: Optional[torch.Tensor] = None,
                   n_groups: Optional[int] = None) -> Optional[Groups]:
    """Launch bgnn_group_plan (asynchronous) or return None when plans are off / unsupported."""
    rows = GROUP_ROWS if rows is None else rows
    if rows <= 0 or chunk > 64 or n_rows == 0:
        return None
    dev = rowptr.device
    G = int(n_groups) if grow is not None else (n_rows + rows - 1) // rows
    gsrc = torch.empty(max(nnz, 1), dtype=torch.int32, device=dev)
    gmask = torch.empty(max(nnz, 1), dtype=torch.uint8, device=dev)
    gcnt = torch.empty(max(G, 1), dtype=torch.int32, device=dev)
    _lib.call("bgnn_group_plan", rowptr.data_ptr(), col.data_ptr(), n_rows, chunk, rows, _ptr(grow), G,
              gsrc.data_ptr(), gmask.data_ptr(), gcnt.data_ptr(), _stream())
    return Groups(gsrc, gmask, gcnt, rows, grow, G)


@dataclass
class Csr:
    rowptr: torch.Tensor
    col: torch.Tensor
    n_rows: int
    nnz: int
    plan: Plan
    groups: Optional[Groups] = None
    _struct: Optional[_lib.CsrStruct] = field(default=None, repr=False)
    # heavy-row ranges (bgnn_heavy_ranges, ensure_ranges): None until requested; ranges_all = 1 when
    # every heavy row is a range row, 0 when not, -1 unknown (ensure_ranges reads it back once)
    ranges: Optional[torch.Tensor] = field(default=None, repr=False)
    ranges_all: int = -1

    def struct(self) -> _lib.CsrStruct:
        if self._struct is None:
            p = self.plan
            assert p.n_heavy >= 0, "plan counts not resolved (call resolve())"
            gr = self.groups
            self._struct = _lib.CsrStruct(
                self.rowptr.data_ptr(), self.col.data_ptr(), p.heavy_row.data_ptr(),
                p.heavy_chunk0.data_ptr(), p.chunk_heavy.data_ptr(), self.n_rows, self.nnz,
                p.n_heavy, p.n_chunks, p.chunk, max(self.ranges_all, 0) if self.ranges is not None else 0,
                gr.gsrc.data_ptr() if gr else None, gr.gmask.data_ptr() if gr else None,
                gr.gcnt.data_ptr() if gr else None, _ptr(gr.grow) if gr else None,
                gr.n_groups if gr else 0, gr.rows if gr else 0, 0, _ptr(self.ranges))
        return self._struct

    def ensure_ranges(self) -> Optional[torch.Tensor]:
        """The heavy rows' source ranges (bgnn_heavy_ranges; include/bgnn.h): a super node wired to
        its graph's contiguous real-node range is a "range row", whose aggregation the row passes
        sum as a by-product (ranges.hip). Computed once per CSR; when ranges_all is not known (no
        GraphStore hint) it is read back with one host sync."""
        p = self.plan
        if p.n_heavy <= 0:
            return None
        if self.ranges is None:
            buf = torch.empty(_lib.query("bgnn_heavy_ranges_bytes", p.n_heavy) // 4, dtype=torch.int32,
                              device=self.rowptr.device)
            self._struct = None
            _lib.call("bgnn_heavy_ranges", self.ref(), buf.data_ptr(), _stream())
            self.ranges = buf
            if self.ranges_all < 0:
                self.ranges_all = int(int(buf[0].item()) == p.n_heavy)
            self._struct = None
        return self.ranges

    def ref(self):
        return ctypes.byref(self.struct())

    def degree(self) -> torch.Tensor:
        return (self.rowptr[1:] - self.rowptr[:-1])


@dataclass
class Graph:
    """Forward CSR (rows = targets) + transpose CSR (rows = sources) of an edge_index."""

    num_nodes: int
    num_edges: int
    fwd: Csr
    bwd: Csr
    perm_t: torch.Tensor
    edge_index: Optional[torch.Tensor] = field(default=None, repr=False)
    meta: Optional[torch.Tensor] = field(default=None, repr=False)   # device int32[5]: status, counts

    @staticmethod
    def enqueue(edge_index: torch.Tensor, num_nodes: int, chunk: int = DEFAULT_CHUNK) -> "Graph":
        """Launch every build kernel without any host synchronisation; call resolve(meta_host)."""
        require_cuda(edge_index, what="Graph.build")
        if edge_index.dim() != 2 or edge_index.size(0) != 2:
            raise ValueError(f"edge_index must have shape [2, E], got {tuple(edge_index.shape)}")
        ei = edge_index.to(torch.int64).contiguous()
        E = ei.size(1)
        N = int(num_nodes)
        dev = ei.device
        meta = torch.zeros(5, dtype=torch.int32, device=dev)
        rowptr = torch.empty(N + 1, dtype=torch.int32, device=dev)
        rowptr_t = torch.empty(N + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        col_t = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        perm_t = torch.empty(max(E, 1), dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.query("bgnn_graph_build_ws_bytes", E, N), dtype=torch.uint8, device=dev)
        _lib.call("bgnn_graph_build", ei.data_ptr(), E, N, rowptr.data_ptr(), col.data_ptr(),
                  rowptr_t.data_ptr(), col_t.data_ptr(), perm_t.data_ptr(), ws.data_ptr(), ws.numel(),
                  meta.data_ptr(), _stream())
        fwd = Csr(rowptr, col, N, E, enqueue_plan(rowptr, N, E, meta[1:3], chunk),
                  enqueue_groups(rowptr, col, N, E, chunk))
        bwd = Csr(rowptr_t, col_t, N, E, enqueue_plan(rowptr_t, N, E, meta[3:5], chunk),
                  enqueue_groups(rowptr_t, col_t, N, E, chunk))
        return Graph(N, E, fwd, bwd, perm_t, edge_index, meta)

    def resolve(self, meta_host) -> "Graph":
        if int(meta_host[0]) != 0:
            raise IndexError(f"edge_index contains indices outside [0, {self.num_nodes})")
        self.fwd.plan.n_heavy, self.fwd.plan.n_chunks = int(meta_host[1]), int(meta_host[2])
        self.bwd.plan.n_heavy, self.bwd.plan.n_chunks = int(meta_host[3]), int(meta_host[4])
        return self

    @staticmethod
    def build(edge_index: torch.Tensor, num_nodes: int, chunk: int = DEFAULT_CHUNK) -> "Graph":
        g = Graph.enqueue(edge_index, num_nodes, chunk)
        return g.resolve(g.meta.tolist())


@dataclass
class SegmentIndex:
    """CSR of `index -> positions` (global_mean_pool's batch, scatter's index) + its transpose."""

    n: int
    num_rows: int
    fwd: Csr          # rows = segments (graphs), col = positions
    bwd: Csr          # rows = positions, exactly one entry: its segment
    index: Optional[torch.Tensor] = field(default=None, repr=False)   # int64 [n]
    meta: Optional[torch.Tensor] = field(default=None, repr=False)    # device int32[3]

    @staticmethod
    def enqueue(index: torch.Tensor, num_rows: int, chunk: int = DEFAULT_CHUNK) -> "SegmentIndex":
        require_cuda(index, what="SegmentIndex.build")
        idx = index.to(torch.int64).contiguous().view(-1)
        n = idx.numel()
        R = int(num_rows)
        dev = idx.device
        meta = torch.zeros(3, dtype=torch.int32, device=dev)
        rowptr = torch.empty(R + 1, dtype=torch.int32, device=dev)
        col = torch.empty(max(n, 1), dtype=torch.int32, device=dev)
        ws = torch.empty(_lib.query("bgnn_graph_build_ws_bytes", n, R), dtype=torch.uint8, device=dev)
        _lib.call("bgnn_index_csr_build", idx.data_ptr(), n, R, rowptr.data_ptr(), col.data_ptr(),
                  ws.data_ptr(), ws.numel(), meta.data_ptr(), _stream())
        fwd = Csr(rowptr, col, R, n, enqueue_plan(rowptr, R, n, meta[1:3], chunk))
        rowptr_t = torch.arange(n + 1, dtype=torch.int32, device=dev)
        col_t = idx.to(torch.int32)
        empty = Plan(torch.zeros(1, dtype=torch.int32, device=dev), torch.zeros(2, dtype=torch.int32, device=dev),
                     torch.zeros(1, dtype=torch.int32, device=dev), 0, 0, chunk)
        bwd = Csr(rowptr_t, col_t if n > 0 else torch.zeros(1, dtype=torch.int32, device=dev), n, n, empty)
        return SegmentIndex(n, R, fwd, bwd, idx, meta)

    def resolve(self, meta_host) -> "SegmentIndex":
        if int(meta_host[0]) != 0:
            raise IndexError(f"index contains values outside [0, {self.num_rows})")
        self.fwd.plan.n_heavy, self.fwd.plan.n_chunks = int(meta_host[1]), int(meta_host[2])
        return self

    @staticmethod
    def build(index: torch.Tensor, num_rows: int, chunk: int = DEFAULT_CHUNK) -> "SegmentIndex":
        s = SegmentIndex.enqueue(index, num_rows, chunk)
        return s.resolve(s.meta.tolist())


class _Cache:
    """Small identity cache: structure built once per distinct index tensor (and version)."""

    def __init__(self, size: int = 8):
        self.size = size
        self.items = []  # list of (tensor, version, key, value)

    def get(self, t: torch.Tensor, key, builder):
        ver = t._version
        for i, (tt, v, k, val) in enumerate(self.items):
            if tt is t and v == ver and k == key:
                if i:
                    self.items.insert(0, self.items.pop(i))
                return val
        val = builder()
        self.items.insert(0, (t, ver, key, val))
        del self.items[self.size:]
        return val

    def peek(self, t: torch.Tensor, key):
        ver = t._version
        for tt, v, k, val in self.items:
            if tt is t and v == ver and k == key:
                return val
        return None

    def put(self, t: torch.Tensor, key, val):
        self.items.insert(0, (t, t._version, key, val))
        del self.items[self.size:]

    def clear(self):
        self.items.clear()


_graph_cache = _Cache()
_index_cache = _Cache(16)   # (a super-node store batch holds three entries: batch, readout, real nodes)
_empty_csrs = {}


def empty_csr(n_rows: int, device) -> Csr:
    """A CSR of n_rows rows without entries (cached per size and device). bgnn_sage_fwd over it
    is the SAGE row epilogue alone -- o_i = normalize(z_r[i] + b), its norm and the BatchNorm
    partial sums -- which the aggregate-first max-aggregation layer (bgnn.fused) applies to its
    GEMM output."""
    key = (int(n_rows), str(device))
    c = _empty_csrs.get(key)
    if c is None:
        if len(_empty_csrs) > 8:
            _empty_csrs.clear()
        dev = torch.device(device)
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        plan = Plan(z, torch.zeros(2, dtype=torch.int32, device=dev), z, 0, 0, DEFAULT_CHUNK)
        c = _empty_csrs[key] = Csr(torch.zeros(n_rows + 1, dtype=torch.int32, device=dev), z, n_rows, 0, plan)
    return c


_identity_csrs = {}


def identity_csr(n_rows: int, device) -> Csr:
    """The CSR of the identity (row i holds the one entry i; cached per size and device, no heavy rows,
    no row-group plan). bgnn_sage_fwd_bf16 (sum) over it adds the two planes of z row by row,
    h_i = (z_l[i] + z_r[i]) + b, and runs the SAGE row epilogue: the bf16 max-aggregation layer's
    tail (bgnn.fused._max_rows_fwd_bf16)."""
    key = (int(n_rows), str(device))
    c = _identity_csrs.get(key)
    if c is None:
        if len(_identity_csrs) > 8:
            _identity_csrs.clear()
        dev = torch.device(device)
        z = torch.zeros(1, dtype=torch.int32, device=dev)
        plan = Plan(z, torch.zeros(2, dtype=torch.int32, device=dev), z, 0, 0, DEFAULT_CHUNK)
        rowptr = torch.arange(n_rows + 1, dtype=torch.int32, device=dev)
        c = _identity_csrs[key] = Csr(rowptr, rowptr, n_rows, n_rows, plan)
    return c


def graph_for(edge_index: torch.Tensor, num_nodes: int, chunk: int = DEFAULT_CHUNK) -> Graph:
    return _graph_cache.get(edge_index, (int(num_nodes), chunk),
                            lambda: Graph.build(edge_index, num_nodes, chunk))


def segments_for(index: torch.Tensor, num_rows: int, chunk: int = DEFAULT_CHUNK) -> SegmentIndex:
    return _index_cache.get(index, (int(num_rows), chunk),
                            lambda: SegmentIndex.build(index, num_rows, chunk))


def host_plan_pack(rowptr_h, chunk: int):
    """The heavy-row plan of a CSR whose rowptr the host holds, as one int32 array
    [heavy rows ascending | heavy_chunk0 = running chunk counts | chunk -> heavy row] -- what
    bgnn_heavy_plan writes -- with the two counts: (pack, n_heavy, n_chunks); an empty pack when no
    row has more than `chunk` entries."""
    deg = np.diff(np.asarray(rowptr_h, dtype=np.int64))
    heavy = np.nonzero(deg > chunk)[0]
    if heavy.size == 0:
        return np.zeros(0, dtype=np.int32), 0, 0
    nch = (deg[heavy] + chunk - 1) // chunk
    c0 = np.concatenate([[0], np.cumsum(nch)])
    ch = np.repeat(np.arange(heavy.size), nch)
    return np.concatenate([heavy, c0, ch]).astype(np.int32), int(heavy.size), int(c0[-1])


def plan_of_pack(d: Optional[torch.Tensor], h: int, n_chunks: int, chunk: int, none: torch.Tensor) -> Plan:
    """The Plan over an uploaded host_plan_pack (d: device int32); none: the int32 placeholder (two
    zeros) of a plan without heavy rows."""
    if h == 0:
        return Plan(none, none, none, 0, 0, chunk)
    return Plan(d[:h], d[h:2 * h + 1], d[2 * h + 1:2 * h + 1 + n_chunks], h, n_chunks, chunk)


def host_plan(rowptr_h, chunk: int, device, none: Optional[torch.Tensor] = None) -> Plan:
    """Heavy-row plan of a CSR whose rowptr the host holds (pooling segments: a row per graph),
    computed in numpy (host_plan_pack) and uploaded in one pinned copy. none: the int32 placeholder
    of a plan without heavy rows (two zeros; made here when not given)."""
    pack, h, n_chunks = host_plan_pack(rowptr_h, chunk)
    if h == 0:
        return plan_of_pack(None, 0, 0, chunk,
                            none if none is not None else torch.zeros(2, dtype=torch.int32, device=device))
    d = torch.from_numpy(pack).pin_memory().to(device, non_blocking=True)
    return plan_of_pack(d, h, n_chunks, chunk, none)


def readout_rowptrs(n_nodes):
    """Host rowptrs of a super-node batch's readout segments from its per-graph node counts: the 2B
    segments [real nodes | super node] per graph (as bgnn_readout_index writes rowptr2) and the B
    real-node segments."""
    n_nodes = np.asarray(n_nodes, dtype=np.int64)
    B = n_nodes.size
    dn = np.concatenate([[0], np.cumsum(n_nodes)])
    rp2 = np.empty(2 * B + 1, dtype=np.int64)
    rp2[0::2], rp2[1::2] = dn, dn[1:] - 1
    return rp2, dn - np.arange(B + 1)


@dataclass
class Readout:
    """The readout index of a batch whose graphs each end in their super node
    (VirtualEdgeCreate.py:106-107), from one bgnn_readout_index launch. seg: the SegmentIndex of 2B
    segments [real nodes of graph 0 | super node of graph 0 | real nodes of graph 1 | ...] over the N
    rows, each listed once: the pool bgnn_sage_apply_pool takes, whose even rows are the real-node
    means and odd rows the super rows. real_index / real_batch: the real nodes' rows and graphs;
    real_seg: the SegmentIndex of real_batch (B segments), also in _index_cache under real_batch."""

    seg: SegmentIndex
    real_index: torch.Tensor
    real_batch: torch.Tensor
    real_seg: SegmentIndex


def build_readout(batch: torch.Tensor, ptr: torch.Tensor, n_nodes, chunk: int = DEFAULT_CHUNK, arange=None,
                  none: Optional[torch.Tensor] = None, plans=None) -> Readout:
    """Build and register the readout index of `batch` (Readout; readout_for finds it). ptr: the
    batch's device int64 [B + 1]; n_nodes: the host's per-graph node counts, from which the
    heavy-segment plans come (host_plan over readout_rowptrs): no sort and no read-back.
    arange(n): an int32 device arange of at least n elements (a cache; a fresh one when None).
    plans: the two plans (2B segments, real-node segments) where the caller uploaded them already."""
    require_cuda(batch, ptr, what="build_readout")
    n_nodes = np.asarray(n_nodes, dtype=np.int64)
    B = int(n_nodes.size)
    if B == 0 or int(n_nodes.min()) < 1:
        raise ValueError("build_readout: every graph needs at least its super node")
    dn = np.concatenate([[0], np.cumsum(n_nodes)])
    N = int(dn[-1])
    if batch.numel() != N or ptr.numel() != B + 1:
        raise ValueError("build_readout: batch / ptr do not match the node counts")
    dev = batch.device
    ptr = ptr.to(torch.int64).contiguous()
    rowptr2 = torch.empty(2 * B + 1, dtype=torch.int32, device=dev)
    seg_of_row = torch.empty(N, dtype=torch.int64, device=dev)
    real_index = torch.empty(N - B, dtype=torch.int64, device=dev)
    real_batch = torch.empty(N - B, dtype=torch.int64, device=dev)
    real_rowptr = torch.empty(B + 1, dtype=torch.int32, device=dev)
    _lib.call("bgnn_readout_index", ptr.data_ptr(), B, N, int(n_nodes.min()), int(n_nodes.max()), rowptr2.data_ptr(),
              seg_of_row.data_ptr(), _ptr(real_index) if N > B else None, _ptr(real_batch) if N > B else None,
              real_rowptr.data_ptr(), _stream())
    if arange is None:
        ar = torch.arange(N + 1, dtype=torch.int32, device=dev)
        arange = lambda n: ar   # noqa: E731
    z = none if none is not None else torch.zeros(2, dtype=torch.int32, device=dev)
    if plans is None:
        plans = [host_plan(rp, chunk, dev, z) for rp in readout_rowptrs(n_nodes)]
    empty = Plan(z, z, z, 0, 0, chunk)   # (a transpose has one entry per row: no heavy rows)
    seg = SegmentIndex(N, 2 * B, Csr(rowptr2, arange(N), 2 * B, N, plans[0]),
                       Csr(arange(N + 1), seg_of_row.to(torch.int32), N, N, empty), seg_of_row, None)
    real_seg = SegmentIndex(N - B, B, Csr(real_rowptr, arange(N - B), B, N - B, plans[1]),
                            Csr(arange(N - B + 1), real_batch.to(torch.int32) if N > B else z, N - B, N - B, empty),
                            real_batch, None)
    ro = Readout(seg, real_index, real_batch, real_seg)
    _index_cache.put(batch, ("readout",), ro)
    _index_cache.put(real_batch, ("batch",), real_seg)
    return ro


def readout_for(batch: Optional[torch.Tensor]) -> Optional[Readout]:
    """The readout index registered for this batch vector (GraphStore.batch on a super-node store,
    register_readout), or None: the models then take the path without it."""
    return None if batch is None else _index_cache.peek(batch, ("readout",))


def register_readout(batch: torch.Tensor, ptr: torch.Tensor, chunk: int = DEFAULT_CHUNK) -> Readout:
    """Register the readout index of a host-collated super-node batch (data.Batch: batch.batch,
    batch.ptr): one read-back of ptr per distinct batch tensor, as batch_segments costs. The caller
    vouches that every graph's last node is its super node and no other node is one."""
    ro = readout_for(batch)
    if ro is None:
        p = ptr.detach().to("cpu", torch.int64).numpy()
        ro = build_readout(batch, ptr.to(batch.device), p[1:] - p[:-1], chunk)
    return ro


def clear_caches() -> None:
    _graph_cache.clear()
    _index_cache.clear()


def prepare(edge_index: torch.Tensor, num_nodes: int, batch: Optional[torch.Tensor] = None,
            num_graphs: Optional[int] = None, chunk: int = DEFAULT_CHUNK):
    """Build (or fetch from cache) the graph structure of a mini-batch and the segment
    structure of its `batch` vector with ONE host synchronisation for all status words and
    plan counts, and register them in the caches used by SAGEConv / BuckGNN / pooling."""
    key = (int(num_nodes), chunk)
    g = _graph_cache.peek(edge_index, key)
    s = None
    pending = []
    if g is None:
        g = Graph.enqueue(edge_index, num_nodes, chunk)
        pending.append(g)
    if batch is not None:
        s = _index_cache.peek(batch, ("batch",))
        if s is None:
            n = num_graphs if num_graphs is not None else int(batch.max().item()) + 1
            s = SegmentIndex.enqueue(batch, n, chunk)
            pending.append(s)
    if pending:
        host = torch.cat([p.meta for p in pending]).tolist()
        off = 0
        for p in pending:
            k = p.meta.numel()
            p.resolve(host[off:off + k])
            off += k
        if pending[0] is g:
            _graph_cache.put(edge_index, key, g)
        if s is not None and pending[-1] is s:
            _index_cache.put(batch, ("batch",), s)
    return g, s
