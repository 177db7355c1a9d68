"""The persistent HEX8 projection kernels under forced schedules (tests/iso_schedule_cases.py has the cases and the
child process).  One child per knob set - the switches are read once per process.  The oracle results are computed
once per module and handed to the children as an .npz; a baseline child without any switch records the projection
points and hand-over counts every other set has to reproduce exactly.

R2S_ISO_RESIDENT=n / R2S_STRAG_WAVES=n are test hooks of iso_project_hex() (rho2sdf_hip.hip): n persistent wavefronts
of iso_project_hex_pl_kernel / of iso_straggler_kernel, so that on grids of at most 48^3 points a wavefront fetches
many groups, a group spans several items, the four LDS slots are reused, and the lanes of the straggler kernel
refill under quota 64 - what production sizes do all the time and the other parity tests only by accident of timing.
(What no counter shows and no set guarantees: the wait for a free slot - a lane still working from the record four
items back is rare, a planted defect in the slot choice changed 2 of 13824 voxels of tiny_items under few_single only.)
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import iso_schedule_cases as C

pytestmark = pytest.mark.gpu
CHILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "iso_schedule_cases.py")


@pytest.fixture(scope="module")
def reference(pkg, oracle, tmp_path_factory):
    """oracle fields of every case, once: -> path of the .npz the children read"""
    ref = {}
    for name in ("one_item", "distorted", "tiny_items", "tet"):
        X, IEN, rn, nmax = C.build_case(name)
        og = oracle.grid_make(X.min(0), X.max(0), nmax, 3)
        odist, oxp, ost = oracle.eval_distances(X, IEN, rn, C.RHO_T, og, C.BF)
        ref[name + "_dist"], ref[name + "_xp"] = odist, oxp
        ref[name + "_sign"] = oracle.sign_detection(X, IEN, rn, C.RHO_T, og)
        ref[name + "_n_iso_fail"], ref[name + "_n_iso_solves"] = ost["n_iso_fail"], ost["n_iso_solves"]
    path = str(tmp_path_factory.mktemp("iso_schedule") / "oracle.npz")
    np.savez(path, **ref)
    return path


def run_child(set_name, reference, tmp_path):
    """one child process with the environment of the knob set -> (counters per case and call, arrays)"""
    knobs, cases = C.KNOB_SETS[set_name]
    env = {k: v for k, v in os.environ.items() if k not in C.SCHEDULE_VARS}
    env.update(knobs)
    prefix = str(tmp_path / set_name)
    t0 = time.perf_counter()
    r = subprocess.run([sys.executable, CHILD, reference, prefix, ",".join(cases)], env=env, capture_output=True, text=True)
    wall = time.perf_counter() - t0
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or "illegal memory access" in r.stderr:
        # killed by a signal or a GPU fault: start nothing more on this GPU
        pytest.exit(f"{set_name} {knobs}: the child died (status {r.returncode})\n{r.stdout}{r.stderr}", returncode=3)
    assert r.returncode == 0, f"{set_name} {knobs}:\n{r.stdout}{r.stderr}"
    with open(prefix + ".json") as f:
        res = json.load(f)
    print(f"\n[{set_name}] {knobs} child wall {wall:.1f} s (in the child {res['total_seconds']} s; per case {res['seconds']})")
    for case, calls in res["stats"].items():
        c = next(iter(calls.values()))
        print(f"  {case}: items {c['n_items']} chunks {c['n_iso_chunks']} handed over {c['n_iso_straggler']} without KKT point {c['n_iso_fail']}")
    return res["stats"], np.load(prefix + ".npz")


@pytest.fixture(scope="module")
def baseline(pkg, reference, tmp_path_factory):
    """no switch at all: the launch parameters of production.  Also where the cases show what they exist for."""
    stats, arrays = run_child("baseline", reference, tmp_path_factory.mktemp("iso_schedule_baseline"))
    ref = np.load(reference)
    c = stats["one_item"]["first"]
    assert c["n_iso_chunks"] >= 100, c    # one element (its other items are boundary triangles): every group lies inside one item
    assert c["n_iso_straggler"] > 1000, c                                        # a list of thousands of entries
    c = stats["distorted"]["first"]   # (items of 4-16 chunks, so groups straddle them: test_iso_schedule_cpu.py)
    assert 4 * c["n_iso_straggler"] > int(ref["distorted_n_iso_solves"]), c      # (about) half the pairs leave the fast path
    c = stats["tiny_items"]["first"]
    assert c["n_items"] > 8 * 4 and c["n_iso_chunks"] < 2 * c["n_items"], c      # a group of 8 spans more items than there are slots
    return stats, arrays


def test_baseline_matches_the_oracle(baseline):
    """the child itself compares every call with the oracle; here: the counters of a case do not depend on the call"""
    stats, _ = baseline
    for case in ("one_item", "distorted", "tiny_items"):
        calls = stats[case]
        assert len({(c["n_iso_straggler"], c["n_iso_fail"], c["n_iso_chunks"]) for c in calls.values()}) == 1, (case, calls)


@pytest.mark.parametrize("set_name", [s for s in C.KNOB_SETS if s != "baseline"])
def test_forced_schedule(set_name, reference, baseline, tmp_path):
    """one knob set: the child asserts every field against the oracle (fused field and distances bit for bit, projection
    points under the bar of test_parity_gpu, n_iso_fail the oracle's); here the projection points and the hand-over
    counts against the baseline child - a lost or doubled pair shows even when the field survives it - and the
    counters that show the forced path was really taken"""
    knobs, cases = C.KNOB_SETS[set_name]
    stats, arrays = run_child(set_name, reference, tmp_path)
    base_stats, base_arrays = baseline
    for key in arrays.files:
        assert np.array_equal(arrays[key], base_arrays[key]), f"{set_name}: {key} differs from the baseline in {int((arrays[key] != base_arrays[key]).sum())} values"
    for case in cases:
        assert stats[case].keys() == base_stats[case].keys()
        for call, c in stats[case].items():
            b = base_stats[case][call]
            # n_iso_straggler counts the pairs handed over (include/rho2sdf_hip.h), also those an overflowing list left
            # to the sweep; at these sizes the default list holds every result slot, so without R2S_ISO_STRAGGLER_CAP
            # it is the number of entries the list received as well
            assert (c["n_iso_straggler"], c["n_iso_fail"]) == (b["n_iso_straggler"], b["n_iso_fail"]), (set_name, case, call, c, b)
            assert (c["n_items"], c["n_iso_chunks"]) == (b["n_items"], b["n_iso_chunks"]), (set_name, case, call, c, b)
    # ---- the forced path was reached ----
    for case in cases:
        for call, c in stats[case].items():
            if "R2S_ISO_RESIDENT" in knobs:     # the capped machine really loops: more than a group of 8 per wavefront
                assert c["n_iso_chunks"] > 8 * int(knobs["R2S_ISO_RESIDENT"]), (set_name, case, call, c)
            if case in ("one_item", "distorted"):   # the cases with a long list
                if "R2S_STRAG_WAVES" in knobs:  # lanes really refill
                    assert c["n_iso_straggler"] > 64 * int(knobs["R2S_STRAG_WAVES"]), (set_name, case, call, c)
                if "R2S_ISO_STRAGGLER_CAP" in knobs:   # the list really overflows
                    assert c["n_iso_straggler"] > int(knobs["R2S_ISO_STRAGGLER_CAP"]), (set_name, case, call, c)
