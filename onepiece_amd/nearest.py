"""Batches of exact nearest-neighbour queries against one target cloud, and the label transfer built on them: the loop of
KDTree<>::KnnSearch(q, ..., 1) + `dists[0] < max_distance` that the reference's example/GetLabelUsingKDTree.cpp writes per vertex
(Geometry/KDTree.h:147-196).  No arithmetic here: the kernels are csrc/nn_batch.hip, and every call fails loudly without a GPU.

    index = NearestIndex(annotated_points)                 # built once (kdtree.BuildTree)
    idx, d2 = index.Query(model_points, 0.1)               # -1 / +inf where nothing is nearer than the (squared) cutoff
    labels = index.TransferLabels(annotated_labels, model_points, 0.1, default_label=0)

Indices are the ones nanoflann 1.3.2 reports (ties and near ties are re-decided on the host in the tree that library would build), distances its
float32 L2_Simple_Adaptor.  numpy in, numpy out; contiguous CUDA torch tensors are searched in HBM and torch tensors come back.
"""
import ctypes as C

import numpy as np

from . import _lib as L

INF = float("inf")


def _points(a, what):
    """-> (pointer, count, mem, device or None, torch module or None, keep-alive)"""
    if hasattr(a, "data_ptr"):
        import torch
        if not a.is_cuda or not a.is_contiguous() or a.dtype != torch.float32 or a.dim() != 2 or a.shape[1] != 3:
            raise ValueError("%s must be a contiguous [n, 3] float32 CUDA tensor" % what)
        L.torch_ready(a)
        return C.c_void_p(a.data_ptr()), int(a.shape[0]), L.OP_MEM_DEVICE, a.device, torch, a
    p = np.ascontiguousarray(a, np.float32)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("%s must be [n, 3]" % what)
    return C.c_void_p(p.ctypes.data), p.shape[0], L.OP_MEM_HOST, None, None, p


class NearestIndex:
    """op_nn_index: the target cloud and its search grid on the device."""

    def __init__(self, points, device=0):
        ptr, m, mem, dev, _, keep = _points(points, "points")
        if dev is not None and dev.index is not None:
            device = dev.index
        self.size, self.device = m, device
        self._h = C.c_void_p()
        L.check(L.load().op_nn_index_create(ptr, m, mem, device, C.byref(self._h)))

    def close(self):
        if getattr(self, "_h", None):
            L.load().op_nn_index_destroy(self._h)
            self._h = None

    __del__ = close

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def Query(self, queries, max_sq_dist=INF):
        """-> (indices int32 [n], squared distances float32 [n])"""
        ptr, n, mem, dev, torch, keep = _points(queries, "queries")
        if torch is not None:
            idx = torch.empty(n, dtype=torch.int32, device=dev)
            d2 = torch.empty(n, dtype=torch.float32, device=dev)
            pi, pd = C.c_void_p(idx.data_ptr()), C.c_void_p(d2.data_ptr())
        else:
            idx, d2 = np.empty(n, np.int32), np.empty(n, np.float32)
            pi, pd = C.c_void_p(idx.ctypes.data), C.c_void_p(d2.ctypes.data)
        L.check(L.load().op_nn_index_query(self._h, ptr, n, mem, float(max_sq_dist), pi, pd))
        return idx, d2

    def TransferLabels(self, labels, queries, max_sq_dist=INF, default_label=0, return_indices=False):
        """labels: one per target point; integer labels of any width are widened to int32 for the call (uint16 semantic labels included)
        and the result comes back as int32.  -> labels [n] (, indices [n])"""
        ptr, n, mem, dev, torch, keep = _points(queries, "queries")
        if torch is not None:
            if not hasattr(labels, "data_ptr"):
                labels = torch.as_tensor(np.ascontiguousarray(labels).astype(np.int32), device=dev)
            lab = labels.to(device=dev, dtype=torch.int32).contiguous()
            L.torch_ready(lab)
            out = torch.empty(n, dtype=torch.int32, device=dev)
            idx = torch.empty(n, dtype=torch.int32, device=dev) if return_indices else None
            pl, po, pi = C.c_void_p(lab.data_ptr()), C.c_void_p(out.data_ptr()), C.c_void_p(idx.data_ptr()) if return_indices else None
            count = int(lab.numel())
        else:
            lab = np.ascontiguousarray(np.asarray(labels).astype(np.int32))
            out = np.empty(n, np.int32)
            idx = np.empty(n, np.int32) if return_indices else None
            pl, po, pi = C.c_void_p(lab.ctypes.data), C.c_void_p(out.ctypes.data), C.c_void_p(idx.ctypes.data) if return_indices else None
            count = lab.size
        if count != self.size:
            raise ValueError("one label per target point is needed (%d labels, %d points)" % (count, self.size))
        L.check(L.load().op_nn_index_transfer_labels(self._h, pl, ptr, n, mem, float(max_sq_dist), int(default_label), po, pi))
        return (out, idx) if return_indices else out

    def Stats(self):
        """-> (queries answered, tied, doubtful) since the index was created"""
        q, t, d = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
        L.check(L.load().op_nn_index_stats(self._h, C.byref(q), C.byref(t), C.byref(d)))
        return q.value, t.value, d.value


def TransferLabels(target_points, target_labels, query_points, max_sq_dist=INF, default_label=0, device=0):
    """op_transfer_labels: one pass of the example in one call (numpy arrays)."""
    t = np.ascontiguousarray(target_points, np.float32)
    q = np.ascontiguousarray(query_points, np.float32)
    lab = np.ascontiguousarray(np.asarray(target_labels).astype(np.int32))
    if t.ndim != 2 or t.shape[1] != 3 or q.ndim != 2 or q.shape[1] != 3 or lab.size != len(t):
        raise ValueError("points must be [n, 3], one label per target point")
    out = np.empty(len(q), np.int32)
    L.check(L.load().op_transfer_labels(C.c_void_p(t.ctypes.data), C.c_void_p(lab.ctypes.data), len(t), C.c_void_p(q.ctypes.data), len(q), L.OP_MEM_HOST, device,
                                        float(max_sq_dist), int(default_label), C.c_void_p(out.ctypes.data), None))
    return out
