"""The fast HEX8 lane machine with its min / max written as bare hardware instructions (fmin_hw / fmax_hw and their
kin in r2s_device_math.hpp), through the public API against the oracle, bit for bit: dist, sign, sdf and xp.

One jittered mesh of 6^3 elements (random nodal densities, so that hundreds of pairs leave the fast path) on a grid of
40^3 points, run (1) under forced schedules - one or two resident wavefronts of iso_project_hex_pl_kernel, one wavefront
of iso_straggler_kernel - which make the lanes of a wavefront work on different items and send the hand-overs through
one refilling wavefront, with equal hand-over counts between the schedules, and (2) as a slab strictly inside the grid
with true_min on and off, where a lane refills in the middle of a segment with a voxel of another item.

The switches are read once per process: one child process per schedule (this file run as a script is the child).
A host-side check of the helpers' NaN / signed-zero semantics is not here: no exported entry reaches them without
launching the solver.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
RHO_T = 0.5
BF = 1.1
SLAB = dict(k_begin=9, k_end=26)   # strictly inside the 40 planes: the slab cuts the mesh on both sides
SCHEDULES = {
    "default": {},
    "resident1": {"R2S_ISO_RESIDENT": "1"},
    "resident2": {"R2S_ISO_RESIDENT": "2"},
    "strag1": {"R2S_STRAG_WAVES": "1"},
}
SCHEDULE_VARS = ("R2S_ISO_RESIDENT", "R2S_ISO_GROUP", "R2S_ISO_WPS", "R2S_ISO_FREE", "R2S_ISO_CPW", "R2S_ISO_STRAGGLER_CAP",
                 "R2S_STRAG_WAVES", "R2S_STRAG_WPC", "R2S_NO_EARLY_ISO", "R2S_NO_OVERLAP", "R2S_NO_SPECULATION")


def build_case():
    from rho2sdf_jl_amd import synthetic
    X, IEN, _ = synthetic.hex_mesh(6, jitter=.30, seed=20240917)
    rn = np.clip(np.random.default_rng(7).normal(0.5, 0.35, len(X)), 0, 1)
    return X, IEN, rn, synthetic.grid_n_max_for_points(40)


@pytest.fixture(scope="module")
def reference(pkg, oracle, tmp_path_factory):
    """the oracle's fields, once, with true_min off and on -> path of the .npz the children read"""
    X, IEN, rn, nmax = build_case()
    og = oracle.grid_make(X.min(0), X.max(0), nmax, 3)
    ref = {}
    ref["dist"], ref["xp"], st = oracle.eval_distances(X, IEN, rn, RHO_T, og, BF)
    ref["sign"] = oracle.sign_detection(X, IEN, rn, RHO_T, og)
    ref["n_iso_solves"], ref["n_iso_fail"] = st["n_iso_solves"], st["n_iso_fail"]
    with oracle.true_min():
        ref["dist_tm"], ref["xp_tm"], _ = oracle.eval_distances(X, IEN, rn, RHO_T, og, BF)
        ref["sign_tm"] = oracle.sign_detection(X, IEN, rn, RHO_T, og)
    path = str(tmp_path_factory.mktemp("minmax_bounds") / "oracle.npz")
    np.savez(path, **ref)
    return path


@pytest.fixture(scope="module")
def runs(pkg, reference, tmp_path_factory):
    """one child per schedule -> {schedule: counters}; a child asserts every field against the oracle itself"""
    out = {}
    tmp = tmp_path_factory.mktemp("minmax_bounds_runs")
    for name, knobs in SCHEDULES.items():
        env = {k: v for k, v in os.environ.items() if k not in SCHEDULE_VARS}
        env.update(knobs)
        res = str(tmp / (name + ".json"))
        r = subprocess.run([sys.executable, os.path.abspath(__file__), reference, res], env=env, capture_output=True, text=True)
        if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
            pytest.exit(f"{name} {knobs}: the child died (status {r.returncode})\n{r.stdout}{r.stderr}", returncode=3)
        print(r.stdout)
        with open(res) as f:
            out[name] = (r.returncode, r.stdout + r.stderr, json.load(f) if r.returncode == 0 else None)
    return out


@pytest.mark.parametrize("name", list(SCHEDULES))
def test_fields_match_the_oracle_under_forced_schedules(name, runs):
    rc, text, res = runs[name]
    assert rc == 0, f"{name} {SCHEDULES[name]}:\n{text}"
    base = runs["default"][2]
    assert base is not None
    # the straggler path is exercised, and no schedule loses or doubles a hand-over
    assert res["full"]["n_iso_straggler"] >= 300, res
    for call in res:
        assert res[call]["n_iso_straggler"] == base[call]["n_iso_straggler"], (name, call, res[call], base[call])
        assert res[call]["n_iso_fail"] == base[call]["n_iso_fail"], (name, call, res[call], base[call])


# ---------------------------------------------------------------------------------------------------------------------
# the child
# ---------------------------------------------------------------------------------------------------------------------
def _equal(label, got, want):
    n = int((got != want).sum())
    print(f"{label}: {n} of {want.size} values differ from the oracle")
    return n == 0


def child(ref_path, out_path):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    sys.path.insert(0, root)
    import torch
    import __graft_entry__ as graft
    pkg = graft.load_built()
    ref = np.load(ref_path)
    X, IEN, rn, nmax = build_case()
    pg = pkg.Grid(X.min(0), X.max(0), nmax, 3)
    nx, ny, nz = pg.dims
    dev = torch.device("cuda:0")
    dX, dI, dR = (torch.from_numpy(np.ascontiguousarray(a)).to(dev) for a in (X, IEN, rn))
    keep = lambda st: {k: int(st[k]) for k in ("n_items", "n_iso_chunks", "n_iso_straggler", "n_iso_fail")}
    stats, ok = {}, True
    plan = pkg.DevicePlan(0)
    # (1) the whole grid: dist, sign, xp in one call, then the fused field
    d, s, f = (torch.empty(pg.ngp, dtype=torch.float64, device=dev) for _ in range(3))
    xp = torch.empty((pg.ngp, 3), dtype=torch.float64, device=dev)
    stats["full"] = keep(plan.run(dX, dI, dR, RHO_T, pg, dist=d, sign=s, xp=xp))
    stats["fused"] = keep(plan.run(dX, dI, dR, RHO_T, pg, sdf=f))
    ok &= _equal("dist", d.cpu().numpy(), ref["dist"])
    ok &= _equal("sign", s.cpu().numpy(), ref["sign"])
    ok &= _equal("xp", xp.cpu().numpy(), ref["xp"])
    ok &= _equal("sdf", f.cpu().numpy(), ref["dist"] * ref["sign"])
    # (2) a slab strictly inside the grid, true_min off and on
    planes = np.arange(SLAB["k_begin"], SLAB["k_end"])
    for tm, sfx in ((False, ""), (True, "_tm")):
        n = len(planes) * ny * nx
        d, s, f = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))
        xp = torch.empty((n, 3), dtype=torch.float64, device=dev)
        stats["slab" + sfx] = keep(plan.run(dX, dI, dR, RHO_T, pg, dist=d, sign=s, xp=xp, true_min=tm, **SLAB))
        stats["slab_fused" + sfx] = keep(plan.run(dX, dI, dR, RHO_T, pg, sdf=f, true_min=tm, **SLAB))
        cut = lambda a: a.reshape((nz, ny, nx) + a.shape[1:])[planes].reshape((n,) + a.shape[1:])
        ok &= _equal("slab dist" + sfx, d.cpu().numpy(), cut(ref["dist" + sfx]))
        ok &= _equal("slab sign" + sfx, s.cpu().numpy(), cut(ref["sign" + sfx]))
        ok &= _equal("slab xp" + sfx, xp.cpu().numpy(), cut(ref["xp" + sfx]))
        ok &= _equal("slab sdf" + sfx, f.cpu().numpy(), cut(ref["dist" + sfx] * ref["sign" + sfx]))
    plan.close()
    for call, c in stats.items():
        print(call, c)
        ok &= c["n_iso_fail"] <= c["n_iso_straggler"] <= int(ref["n_iso_solves"])
    with open(out_path, "w") as fo:
        json.dump(stats, fo)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(child(sys.argv[1], sys.argv[2]))
