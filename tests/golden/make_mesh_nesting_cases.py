"""Writes tests/golden/mesh_nesting_tris.npz (or the path given as the first argument): the triangles of the library's own
iso-surface extraction (r2s_extract_isosurface, needs a GPU) for the fields of tests/mesh_nesting_cases.py.  Only the triangles
are recorded; the vertices are restated by tests/iso_ref.py, and this script checks that they agree bit for bit."""
import ctypes
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import __graft_entry__ as graft  # noqa: E402
import iso_ref as R  # noqa: E402
import mesh_nesting_cases as C  # noqa: E402


def extract(pkg, n, f):
    L = pkg._lib
    nv, nt = ctypes.c_int64(), ctypes.c_int64()
    L.check(L.lib().r2s_extract_isosurface(f.ctypes.data_as(ctypes.c_void_p), 1, (ctypes.c_int64 * 3)(n, n, n),
                                           (ctypes.c_double * 3)(*C.ORIGIN), C.SPACING, 0.0, -1, None, 0, None, 0, ctypes.byref(nv),
                                           ctypes.byref(nt)))
    return pkg.api._last_isosurface()


def main(pkg, path):
    out = {}
    for name, (n, f) in C.fields().items():
        V, T = extract(pkg, n, np.ascontiguousarray(f, np.float32))
        Vr, _ = R.vertices(f, (n, n, n), C.ORIGIN, C.SPACING, 0.0)
        assert V.shape == Vr.shape and (V.view(np.uint32) == Vr.view(np.uint32)).all(), name
        out[name] = T
        print(name, len(V), "vertices", len(T), "triangles")
    np.savez_compressed(path, **out)


if __name__ == "__main__":
    main(graft.build(), sys.argv[1] if len(sys.argv) > 1 else C.GOLDEN)
