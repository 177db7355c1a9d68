"""The meshes and element densities of the pre-stage reference tests (CPU and GPU files share them).

Seeds are fixed; tests/test_pre_reference_cpu.py checks with the float64 reference alone that every case stays inside the
caps on undecidable nodes and flagged Gauss weight, and that together the cases reach every leg of DenseInNodes and
LamReduction."""
import os
import sys

import numpy as np

from conftest import load_fixture

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as graft  # noqa: E402

FIXTURES = ("sphere", "beam_vfrac_03", "chapadlo")
# translation: cancellation in A'A (other LamReduction legs); (1, 1e-3, 1e3): the ratios cross both thresholds;
# (1, 1e-2, 1e-2), a thin bar: 3e3 < e2 <= e1 < 1e7, the leg that falls through to mean(b)
TRANSFORMS = {
    "id": lambda X: X,
    "+30": lambda X: X + 30.0,
    "+1000": lambda X: X + 1000.0,
    "aniso": lambda X: X * np.array([1.0, 1e-3, 1e3]),
    "bar": lambda X: X * np.array([1.0, 1e-2, 1e-2]),
}
DENSITIES = ("uniform", "constant", "linear", "binary", "ones")


def _syn():
    graft.load_package()
    from rho2sdf_jl_amd import synthetic
    return synthetic


def holes_mesh(n=10, seed=7):
    """a hex mesh with a random third of its elements deleted and the rest shuffled: nodes with 3, 5, 6, 7 elements and
    nodes that no element uses"""
    X, IEN, _ = _syn().hex_mesh(n, 0.15)
    rng = np.random.default_rng(seed)
    keep = rng.permutation(len(IEN))[: (2 * len(IEN)) // 3]
    return X, np.ascontiguousarray(IEN[keep])


def few_elements(kind, nel):
    """the first nel elements of a 2^3 hex mesh (or of its tets), all 27 nodes kept: most nodes belong to no element"""
    syn = _syn()
    X, IEN, _ = syn.hex_mesh(2, 0.15)
    if kind == "tet":
        IEN = syn.hex_to_tets(IEN)
    return X, np.ascontiguousarray(IEN[:nel])


def small_cases():
    """name -> (X, IEN) builder, everything but the fixtures and the million-node mesh"""
    syn = _syn()
    out = {}
    for jit in (0.15, 0.45):
        for kind, n, make in (("hex", 12, syn.hex_mesh), ("tet", 8, syn.tet_mesh)):
            for tname, tf in TRANSFORMS.items():
                def build(make=make, n=n, jit=jit, tf=tf):
                    X, IEN, _ = make(n, jit)
                    return np.ascontiguousarray(tf(X)), IEN
                out[f"{kind}{n}-j{jit}-{tname}"] = build
    for kind, n, make in (("hex", 7, syn.hex_mesh), ("tet", 5, syn.tet_mesh)):   # the iso-volume cases: 15^3 points per cut element
        for tname in ("id", "+30", "aniso"):
            def build(make=make, n=n, tf=TRANSFORMS[tname]):
                X, IEN, _ = make(n, 0.3)
                return np.ascontiguousarray(tf(X)), IEN
            out[f"{kind}{n}-j0.3-{tname}"] = build
    out["holes"] = holes_mesh
    for kind in ("hex", "tet"):
        for nel in (1, 2, 3, 5):
            out[f"{kind}-nel{nel}"] = (lambda kind=kind, nel=nel: few_elements(kind, nel))
    return out


def big_mesh():
    """nnp + 1 > 1024 * 1024: the scan of the node -> element counts carries across its 1024-tile passes"""
    X, IEN, _ = _syn().hex_mesh(102, 0.15)
    assert len(X) + 1 > 1024 * 1024
    return X, IEN


def density(kind, X, IEN, seed=11):
    rng = np.random.default_rng(seed)
    nel = len(IEN)
    C = X[IEN - 1].mean(axis=1)
    if kind == "uniform":
        return rng.random(nel)
    if kind == "constant":
        return np.full(nel, 0.37)
    if kind == "linear":
        ext = np.maximum(np.abs(X).max(0), 1e-300)
        return 0.5 + 0.4 * (C / ext) @ np.array([0.5, -0.3, 0.2])
    if kind == "binary":
        return (rng.random(nel) < 0.4).astype(np.float64)
    if kind == "ones":
        return np.ones(nel)
    raise KeyError(kind)


def fixture(name):
    X, IEN, rho = load_fixture(name)
    return np.ascontiguousarray(X, dtype=np.float64), IEN, np.asarray(rho, dtype=np.float64)
