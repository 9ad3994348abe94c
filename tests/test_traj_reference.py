"""CPU: the torch restatement of the flow-trajectory chaining (tests/traj_ref.py) against tests/golden/traj.npz, which
make_golden_traj.py wrote from the un-modified reference script; the comparison the GPU tests use rejects planted defects; the new
library entries refuse bad arguments without a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import traj_data as D
import traj_ref as R

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj.npz")
SETTINGS = [(name, direct) for name in D.GOLDEN_CASES for direct in (False, True)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


@pytest.fixture(scope="module")
def cases():
    return {name: make() for name, (make, _) in D.GOLDEN_CASES.items()}


def chain(case, min_len, direct, **kw):
    extra = (lambda s: case["direct"][s], D.DIRECT_THRESHOLD) if direct else (None, None)
    return R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, min_len, *extra, **kw)


def key(name, direct):
    return f"{name}_{'direct' if direct else 'plain'}"


def test_inputs_regenerate(gold, cases):
    for name, case in cases.items():
        assert D.case_digest(case) == str(gold[f"digest_{name}"]), name


@pytest.mark.parametrize("name,direct", [s for s in SETTINGS if s[0].startswith("lattice")])
def test_lattice_restatement_equals_reference_bits(gold, cases, name, direct):
    """every quantity of the lattice case is exact in fp32, so the restatement and the reference agree to the bit"""
    case, min_len = cases[name], D.GOLDEN_CASES[name][1]
    want = torch.from_numpy(gold[f"traj_{key(name, direct)}"])
    assert R.same_bits(chain(case, min_len, direct), want)
    masks = R.consistency_masks(case["fflow"], case["bflow"], D.THRESHOLD)
    assert torch.equal(masks, torch.from_numpy(gold[f"masks_{key(name, direct)}"]))
    ok = ~want.isnan().any(-1)
    assert sorted(set(ok.float().argmax(1).tolist())) == list(range(case["T"] - (min_len - 1)))   # starts at every eligible frame


@pytest.mark.parametrize("direct", [False, True])
def test_smooth_restatement_within_reference_error(gold, cases, direct):
    """same rows, same NaN pattern; coordinates within 4 x ref_dev: ref_dev is how far the reference's fp32 evaluation lies from
    float64, a second fp32 evaluation in another operation order lies about as far on the other side, and the rest is twofold
    slack"""
    case = cases["smooth"]
    want = torch.from_numpy(gold[f"traj_{key('smooth', direct)}"])
    ok, dev = R.same_pattern_within(chain(case, 2, direct), want, 4 * float(gold["ref_dev"]))
    print(f"smooth direct={direct}: fp32 restatement vs reference {dev:.3g} px, bound {4 * float(gold['ref_dev']):.3g}")
    assert ok, dev
    masks = R.consistency_masks(case["fflow"], case["bflow"], D.THRESHOLD)
    assert torch.equal(masks, torch.from_numpy(gold[f"masks_{key('smooth', direct)}"]))


def test_direct_filter_changes_the_rows(gold):
    for name in D.GOLDEN_CASES:
        a, b = gold[f"traj_{key(name, False)}"], gold[f"traj_{key(name, True)}"]
        assert a.shape != b.shape or not np.array_equal(a, b, equal_nan=True), name
    assert abs(gold["traj_smooth_plain"].shape[0] - gold["traj_smooth_direct"].shape[0]) >= 20


@pytest.mark.parametrize("defect", R.DEFECTS)
@pytest.mark.parametrize("direct", [False, True])
def test_planted_defect_is_rejected(gold, cases, defect, direct):
    """the bit comparison of the GPU tests (trajectories and masks against the fp32 restatement / the lattice golden) fails for a
    restatement with one deviation planted"""
    case = cases["lattice"]
    want = torch.from_numpy(gold[f"traj_{key('lattice', direct)}"])
    assert not R.same_bits(chain(case, 2, direct, defect=defect), want), defect
    if defect in ("le", "round_away", "border"):   # these also show in the masks
        masks = R.consistency_masks(case["fflow"], case["bflow"], D.THRESHOLD, defect=defect)
        assert not torch.equal(masks, torch.from_numpy(gold[f"masks_{key('lattice', direct)}"])), defect


def test_float64_margin_is_recorded(gold, cases):
    """the float64 run reports the smallest decision margin; it is the one stored with the golden"""
    m = R.Margin()
    for direct in (False, True):
        chain(cases["smooth"], 2, direct, dtype=torch.float64, margin=m)
    assert m.value == pytest.approx(float(gold["margin"]), rel=1e-6) and m.value > float(gold["ref_dev"])


def test_library_refuses_bad_arguments_without_a_device():
    import __graft_entry__ as entry
    from dino_tracker_amd import _lib
    entry.build()
    h = _lib.lib()
    err = lambda: h.dtk_last_error().decode()   # noqa: E731
    one = ctypes.c_void_p(1)   # never dereferenced: every call below must fail before it reaches the device
    assert h.dtk_flow_pack(None, one, 3, 8, 8, None) == -1 and "null pointer" in err()
    assert h.dtk_flow_pack(one, one, 3, 0, 8, None) == -1 and "bad sizes" in err()
    assert h.dtk_flow_cycle_masks(one, one, 1, 8, 8, 1.0, one, None) == -1 and "T >= 2" in err()
    assert h.dtk_flow_cycle_masks(one, None, 4, 8, 8, 1.0, one, None) == -1 and "null pointer" in err()
    assert h.dtk_flow_traj_workspace_bytes(1, 8, 8) == 0 and h.dtk_flow_traj_workspace_bytes(4, 1, 8) == 0
    nb = h.dtk_flow_traj_workspace_bytes(4, 8, 8)
    assert nb >= 4 * 64 * 8 + 2 * 64 * 4

    def start(T=4, s=0, min_len=2, fpk=one, df=None, db=None, use=0, n_rows=one, ws=one, ws_bytes=nb):
        return h.dtk_flow_traj_start(fpk, one, one, one, T, 8, 8, s, 1.0, min_len, df, db, use, 1.5, n_rows, ws, ws_bytes, None)

    assert start(T=1) == -1 and "T >= 2" in err()
    assert start(s=4) == -1 and "starting frame" in err()
    assert start(min_len=0) == -1 and "min_trajectory_length" in err()
    assert start(min_len=5) == -1 and "min_trajectory_length" in err()
    assert start(fpk=None) == -1 and "null pointer" in err()
    assert start(use=1) == -1 and "direct-flow threshold without direct flows" in err()
    assert start(df=one, db=one) == -1 and "direct flows without a direct-flow threshold" in err()
    assert start(ws_bytes=nb - 1) < 0 and "workspace" in err()

    def emit(T=4, s=0, min_len=2, n=1, rows=one, vis=one, ws_bytes=nb):
        return h.dtk_flow_traj_emit(T, 8, 8, s, min_len, n, rows, vis, one, ws_bytes, None)

    assert emit(T=1) == -1 and "T >= 2" in err()
    assert emit(min_len=5) == -1 and "min_trajectory_length" in err()
    assert emit(n=65) == -1 and "n_rows" in err()
    assert emit(rows=None) == -1 and "null pointer" in err()
    assert emit(ws_bytes=8) < 0 and "workspace" in err()


def test_python_entry_rejects_half_a_direct_filter():
    from dino_tracker_amd import flow_trajectories as FT
    f = torch.zeros(3, 2, 8, 8)
    with pytest.raises(ValueError, match="come together"):
        FT.chain_trajectories(f, f, direct_flows=lambda s: (f, f))
    with pytest.raises(ValueError, match="come together"):
        FT.chain_trajectories(f, f, direct_flow_threshold=1.5)
