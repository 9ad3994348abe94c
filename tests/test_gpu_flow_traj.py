"""GPU: the device flow-trajectory chaining (dino_tracker_amd.flow_trajectories on dtk_flow_*) equals the fp32 restatement of
tests/traj_ref.py, evaluated on the CPU at test time, BIT FOR BIT -- trajectories (NaN rows included) and consistency masks, with
and without the direct-flow filter -- and the goldens the un-modified reference script wrote (tests/golden/traj.npz): bit for bit
on the lattice case, within the CPU test's bound on the smooth one.  Edge cases and the command line follow."""
import os

import numpy as np
import pytest
import torch

import traj_data as D
import traj_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "traj.npz")
# name -> (case maker, min_trajectory_length); "mid" (T = 12, 120 x 200: 94 blocks of 256 pixels, 12 frames in one 16-frame
# tile) crosses the block boundaries of the scans and the transpose
CASES = dict(D.GOLDEN_CASES, mid=(lambda: D.smooth(**D.MID), 2))
SETTINGS = [(name, direct) for name in CASES for direct in (False, True)]


@pytest.fixture(scope="module")
def gold():
    return dict(np.load(GOLD))


_cases, _refs = {}, {}


def case_of(name):
    if name not in _cases:
        _cases[name] = CASES[name][0]()
    return _cases[name]


def direct_args(case, direct):
    return (lambda s: case["direct"][s], D.DIRECT_THRESHOLD) if direct else (None, None)


def restated(name, direct):
    """the fp32 restatement on the CPU, computed once per setting and never modified"""
    if (name, direct) not in _refs:
        case = case_of(name)
        _refs[name, direct] = R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, CASES[name][1],
                                                   *direct_args(case, direct))
    return _refs[name, direct]


def device_chain(case, min_len, direct, **kw):
    from dino_tracker_amd import flow_trajectories as FT
    return FT.chain_trajectories(torch.from_numpy(case["fflow"]), torch.from_numpy(case["bflow"]), D.THRESHOLD, min_len,
                                 *direct_args(case, direct), device=DEV, **kw)


def key(name, direct):
    return f"{name}_{'direct' if direct else 'plain'}"


@pytest.mark.parametrize("name,direct", SETTINGS)
def test_chain_equals_restatement_bits(gold, name, direct):
    case, min_len = case_of(name), CASES[name][1]
    got = device_chain(case, min_len, direct)
    want = restated(name, direct)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape, (got.shape, want.shape)
    assert R.same_bits(got, want)
    if name.startswith("lattice"):
        assert R.same_bits(got, torch.from_numpy(gold[f"traj_{key(name, direct)}"]))
    elif name == "smooth":
        ok, dev = R.same_pattern_within(got, torch.from_numpy(gold[f"traj_{key(name, direct)}"]), 4 * float(gold["ref_dev"]))
        assert ok, dev


@pytest.mark.parametrize("name", ["lattice", "smooth", "mid"])
def test_consistency_masks_equal_restatement(gold, name):
    from dino_tracker_amd import flow_trajectories as FT
    case = case_of(name)
    got = FT.consistency_masks(torch.from_numpy(case["fflow"]), torch.from_numpy(case["bflow"]), D.THRESHOLD, device=DEV)
    assert got.dtype == torch.bool and got.is_cuda
    assert torch.equal(got.cpu(), R.consistency_masks(case["fflow"], case["bflow"], D.THRESHOLD))
    assert not got[0].any()
    if name != "mid":
        assert torch.equal(got.cpu(), torch.from_numpy(gold[f"masks_{key(name, False)}"]))


@pytest.mark.parametrize("direct", [False, True])
def test_two_frames(direct):
    """T = 2: one starting frame, one step; also min_trajectory_length 1, where the last frame starts rows of one point"""
    case = case_of("lattice")
    two = dict(T=2, h=case["h"], w=case["w"], fflow=case["fflow"][:1], bflow=case["bflow"][:1],
               direct=[(case["fflow"][:1], case["bflow"][:1])])
    for min_len in (2, 1):
        want = R.chain_trajectories(two["fflow"], two["bflow"], D.THRESHOLD, min_len, *direct_args(two, direct))
        got = device_chain(two, min_len, direct)
        assert want.shape[0] > 0 and R.same_bits(got, want), min_len


@pytest.mark.parametrize("direct", [False, True])
def test_everything_leaves_the_image(direct):
    case = D.outward()   # 19 x 27: neither side a multiple of anything
    got = device_chain(case, 2, direct)
    assert got.shape == (0, case["T"], 2) and got.dtype == torch.float32 and got.is_cuda
    assert R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, 2, *direct_args(case, direct)).shape[0] == 0
    # with min_trajectory_length 1 every pixel of every frame is a row of one point
    got = device_chain(case, 1, direct)
    want = R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, 1, *direct_args(case, direct))
    assert want.shape[0] == case["T"] * case["h"] * case["w"] and R.same_bits(got, want)


@pytest.mark.parametrize("direct", [False, True])
def test_min_length_equals_frame_count(direct):
    for name in ("lattice", "smooth"):
        case = case_of(name)
        want = R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, case["T"], *direct_args(case, direct))
        got = device_chain(case, case["T"], direct)
        assert R.same_bits(got, want), name
        assert 0 < got.shape[0] < restated(name, direct).shape[0] and not got.isnan().any(), name


def test_sizes_off_the_block():
    """a width and a height that are no multiple of the 256-pixel block or the 64-lane wave, more frames than one 16-frame tile"""
    case = D.smooth(seed=5, T=19, h=37, w=53)
    for direct in (False, True):
        want = R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, 3, *direct_args(case, direct))
        assert want.shape[0] > 1000 and R.same_bits(device_chain(case, 3, direct), want), direct


def test_wrappers_refuse_bad_input():
    from dino_tracker_amd import flow_trajectories as FT
    case = case_of("lattice")
    f, b = torch.from_numpy(case["fflow"]), torch.from_numpy(case["bflow"])
    with pytest.raises(ValueError, match="min_trajectory_length"):
        FT.chain_trajectories(f, b, min_trajectory_length=case["T"] + 1, device=DEV)
    with pytest.raises(ValueError, match="differ in shape"):
        FT.chain_trajectories(f, b[:-1], device=DEV)
    with pytest.raises(RuntimeError, match="direct flows of start 0"):
        FT.chain_trajectories(f, b, direct_flows=lambda s: (f[:1], b[:1]), direct_flow_threshold=1.5, device=DEV)


@pytest.mark.parametrize("direct", [False, True])
def test_cli_round_trip(tmp_path, capsys, direct):
    """--flows-path writes chain_trajectories(...).cpu() and prints the reference's line; `of_preprocessing split` takes the file"""
    from PIL import Image
    from dino_tracker_amd import flow_trajectories as FT, of_preprocessing as OP
    case = case_of("smooth")
    flows = {"forward": torch.from_numpy(case["fflow"]), "backward": torch.from_numpy(case["bflow"]),
             "direct": [(torch.from_numpy(a), torch.from_numpy(b)) for a, b in case["direct"]]}
    if not direct:
        del flows["direct"]
    flows_path, out_path = str(tmp_path / "flows.pt"), str(tmp_path / "of_trajectories" / "trajectories.pt")
    torch.save(flows, flows_path)
    argv = ["--output-path", out_path, "--flows-path", flows_path, "--threshold", str(D.THRESHOLD), "--min-trajectory-length", "2"]
    if direct:
        argv += ["--filter-using-direct-flow", "--direct-flow-threshold", str(D.DIRECT_THRESHOLD)]
    FT.main(argv)
    saved = torch.load(out_path)
    assert not saved.is_cuda and R.same_bits(saved, restated("smooth", direct))
    assert f"Saved {out_path}, shape: {saved.shape}" in capsys.readouterr().out
    masks = tmp_path / "masks"
    masks.mkdir()
    m = np.zeros((476, 854), dtype=np.uint8)   # the size load_masks resizes to; the trajectories live in its top left corner
    m[:, : case["w"] // 2] = 255
    for t in range(case["T"]):
        Image.fromarray(m).save(str(masks / f"{t:05d}.png"))
    fg_path, bg_path = str(tmp_path / "fg.pt"), str(tmp_path / "bg.pt")
    OP.main(["split", "--traj_path", out_path, "--fg_masks_path", str(masks), "--fg_traj_path", fg_path, "--bg_traj_path", bg_path])
    fg, bg = torch.load(fg_path), torch.load(bg_path)
    assert fg.shape[0] > 0 and bg.shape[0] > 0 and fg.shape[0] + bg.shape[0] == saved.shape[0]


def test_cli_needs_direct_flows_for_the_filter(tmp_path):
    from dino_tracker_amd import flow_trajectories as FT
    case = case_of("lattice")
    flows_path = str(tmp_path / "flows.pt")
    torch.save({"forward": torch.from_numpy(case["fflow"]), "backward": torch.from_numpy(case["bflow"])}, flows_path)
    with pytest.raises(KeyError, match="direct"):
        FT.main(["--output-path", str(tmp_path / "t.pt"), "--flows-path", flows_path, "--filter-using-direct-flow",
                 "--direct-flow-threshold", "1.5"])
    with pytest.raises(ValueError, match="direct-flow-threshold"):
        FT.main(["--output-path", str(tmp_path / "t.pt"), "--flows-path", flows_path, "--filter-using-direct-flow"])


def test_wide_image_crosses_scan_chunks():
    """300 x 900 = 270 000 pixels: 1 055 blocks of 256, so the one-block scan of the block counts carries across five chunks of
    256 (the headline 476 x 854 has 1 588 blocks), and the repack and the mask clear (1.08 M and 1.35 M elements) stride past
    their 4 096-block grids"""
    from dino_tracker_amd import flow_trajectories as FT
    case = D.smooth(seed=11, T=5, h=300, w=900)
    want = R.chain_trajectories(case["fflow"], case["bflow"], D.THRESHOLD, 2)
    assert want.shape[0] > 270000 and R.same_bits(device_chain(case, 2, False), want)
    masks = FT.consistency_masks(torch.from_numpy(case["fflow"]), torch.from_numpy(case["bflow"]), D.THRESHOLD, device=DEV)
    assert torch.equal(masks.cpu(), R.consistency_masks(case["fflow"], case["bflow"], D.THRESHOLD))


class LookupFlow:
    """a flow_fn that recovers the frame indices painted into the images and looks the seeded flow up; a call whose sources are
    one frame (or whose targets are) asks for direct flows, a call on a consecutive pair both ways for the consecutive ones"""

    def __init__(self, case):
        self.case, self.batches = case, []

    def __call__(self, src, dst):
        i = torch.round(src[:, 0, 0, 0] * 255).long().tolist()
        j = torch.round(dst[:, 0, 0, 0] * 255).long().tolist()
        c = self.case
        pair = len(i) == 2 and i[0] != i[1] and i == j[::-1]
        self.batches.append(("pair" if pair else "direct", len(i)))
        out = []
        for a, b in zip(i, j):
            if pair:
                f = c["fflow"][a] if b > a else c["bflow"][b]
            else:
                f = c["direct"][a][0][b - a - 1] if b > a else c["direct"][b][1][a - b - 1]
            out.append(torch.from_numpy(f))
        return torch.stack(out).to(src.device)


@pytest.mark.parametrize("direct", [False, True])
def test_extract_trajectories_drives_a_flow_fn(direct):
    """the whole driver on a video of 19 frames: consecutive pairs both ways in calls of two, the direct flows of a starting frame
    in chunks of 16 (16 + 2 for the first), the result equal to chain_trajectories on the same flows"""
    from dino_tracker_amd import flow_trajectories as FT
    case = D.smooth(seed=3, T=19, h=12, w=16)
    T = case["T"]
    video = (torch.arange(T, dtype=torch.float32) / 255).view(T, 1, 1, 1).expand(T, 3, case["h"], case["w"]).contiguous()
    fn = LookupFlow(case)
    got = FT.extract_trajectories(video, fn, D.THRESHOLD, 2, filter_using_direct_flow=direct,
                                  direct_flow_threshold=D.DIRECT_THRESHOLD if direct else None, device=DEV)
    want = device_chain(case, 2, direct)
    assert want.shape[0] > 100 and R.same_bits(got, want)
    assert fn.batches[:T - 1] == [("pair", 2)] * (T - 1)
    rest = fn.batches[T - 1:]
    if direct:
        assert rest[:4] == [("direct", 16), ("direct", 2)] * 2 and max(n for _, n in rest) == 16
        assert sum(n for _, n in rest) == 2 * sum(T - 1 - s for s in range(T - 1))
    else:
        assert rest == []
    with pytest.raises(ValueError, match="direct-flow-threshold"):
        FT.extract_trajectories(video, fn, filter_using_direct_flow=True, device=DEV)
