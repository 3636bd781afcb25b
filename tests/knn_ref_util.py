"""The plain-C restatement of the KNearestSearch contract (tests/cpp/knn_ref.c) built into a temporary directory and
loaded with ctypes, and the data sets the knn tests share."""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
NAN_BITS = 0x7FF8000000000000


def build_ref(tmpdir):
    so = os.path.join(str(tmpdir), "knn_ref.so")
    if not os.path.exists(so):
        subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(HERE, "cpp", "knn_ref.c"), "-o",
                        so, "-lm"], check=True)
    L = C.CDLL(so)
    P = C.c_void_p
    L.knn_ref_search.argtypes = [P, C.c_size_t, C.c_int, P, C.c_size_t, C.c_int, C.c_int64, C.c_double, P, P, P, P]
    L.knn_ref_search.restype = None
    return Ref(L)


class Ref:
    def __init__(self, L):
        self.L = L

    def search(self, data, queries, knn, search=0, radius=0.0):
        """data (N, dim), queries (m, dim) -> (indices int64 (m, kout), dist, d2, counts), padded -1 / +inf"""
        data = np.ascontiguousarray(data, np.float64)
        n, dim = data.shape
        q = np.ascontiguousarray(queries, np.float64).reshape(-1, dim)
        m = len(q)
        kout = min(int(knn), n)
        idx = np.zeros((m, kout), np.int64)
        dist = np.zeros((m, kout))
        d2 = np.zeros((m, kout))
        counts = np.zeros(m, np.int64)
        self.L.knn_ref_search(data.ctypes.data, n, dim, q.ctypes.data, m, int(search), int(knn), float(radius),
                              idx.ctypes.data, dist.ctypes.data, d2.ctypes.data, counts.ctypes.data)
        return idx, dist, d2, counts


def bits(a):
    """float64 array -> uint64 bits with every NaN canonical (the contract returns the quiet NaN 0x7FF8...)"""
    a = np.ascontiguousarray(a, np.float64)
    b = a.view(np.uint64).copy()
    b[np.isnan(a)] = NAN_BITS
    return b


def numpy_brute(data, queries, knn):
    """numpy brute force in the contract's order: acc = acc + (q[:, k] - r[k])**2 over k, then lexsort by (d2, index)"""
    data = np.asarray(data, np.float64)
    queries = np.asarray(queries, np.float64).reshape(-1, data.shape[1])
    n = len(data)
    kout = min(knn, n)
    out_i = np.zeros((len(queries), kout), np.int64)
    out_d = np.zeros((len(queries), kout))
    for qi, q in enumerate(queries):
        acc = np.zeros(n)
        for k in range(data.shape[1]):
            d = q[k] - data[:, k]
            acc = acc + d * d
        key = bits(acc)
        order = np.lexsort((np.arange(n), key))[:kout]
        out_i[qi] = order
        out_d[qi] = key[order].view(np.float64)
    return out_i, out_d


def lattice(side, dim=3):
    g = np.stack(np.meshgrid(*[np.arange(side, dtype=np.float64)] * dim, indexing="ij"), -1)
    return g.reshape(-1, dim)
