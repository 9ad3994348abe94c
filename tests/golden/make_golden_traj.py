"""Writes tests/golden/traj.npz by running the UN-MODIFIED reference preprocessing/extract_trajectories.py `save_trajectories` on the
CPU (needs a reference checkout, see oracle/ref_harness.py):
    python tests/golden/make_golden_traj.py

Inputs come from tests/golden/traj_data.py (seeded, bit-identical everywhere; their digests are stored).  The script runs as is; what
it cannot reach on a CPU-only machine without torchvision is stood in for around it:
  * stub modules `torchvision.models` / `torchvision.models.optical_flow` are registered before the import: `raft_large` returns a
    model that LOOKS THE SEEDED FLOW UP by frame index.  Frame i is written as a PNG whose pixels all equal i, so the stub recovers
    the indices from image[b, 0, 0, 0] * 255; it replicate-pads the flow to the padded frame size, and the script's own `unpad`
    crops it back.  While compute_direct_flows_for_start_frame runs, the stub answers with the direct flows.
  * the script always calls resize_flow (its `shape[0] != h` test looks at the batch dimension): the empty cv2 shim gets an identity
    `resize` for equal sizes at run time.
  * torch.Tensor.cuda is bound to the identity for the call, the module's `device` is "cpu", tzip / tqdm are made silent, and
    infer_res_size is None (no Lanczos path).
Stored per case and filter setting: the trajectories and the consistency masks the script computed.  For the smooth case also
`ref_dev`, the largest deviation (over both filter settings) of the reference from the float64 restatement (tests/traj_ref.py)
-- their row sets and NaN patterns must agree for the committed seed (pick another seed in traj_data.SMOOTH if not) -- and
`margin`, the smallest decision margin.
"""
import os
import sys
import tempfile
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests"), HERE):
    if p not in sys.path:
        sys.path.insert(0, p)
from oracle import ref_harness  # noqa: E402
import traj_data as D  # noqa: E402
import traj_ref as R  # noqa: E402

OUT = os.path.join(HERE, "traj.npz")


class FlowLookup:
    """stands in for RAFT: the seeded flow between the two frames whose indices are painted into the images"""

    def __init__(self):
        self.case, self.direct, self.calls = None, False, 0

    def to(self, *a, **k):
        return self

    def eval(self):
        return self

    def __call__(self, src, dst, num_flow_updates=None):
        assert num_flow_updates == 24
        c = self.case
        h, w = c["h"], c["w"]
        ph, pw = src.shape[-2] - h, src.shape[-1] - w
        pad = [pw // 2, pw - pw // 2, ph // 2, ph - ph // 2]   # InputPadder, "sintel" mode
        flows = []
        for a, b in zip(src, dst):
            i, j = int(torch.round(a[0, 0, 0] * 255)), int(torch.round(b[0, 0, 0] * 255))
            assert torch.all(a == a[0, 0, 0]) and torch.all(b == b[0, 0, 0]) and i != j
            if self.direct:
                f = c["direct"][i][0][j - i - 1] if j > i else c["direct"][j][1][i - j - 1]
            else:
                assert abs(i - j) == 1
                f = c["fflow"][i] if j > i else c["bflow"][j]
            flows.append(torch.from_numpy(np.ascontiguousarray(f)))
        self.calls += 1
        flow = torch.nn.functional.pad(torch.stack(flows), pad, mode="replicate")
        return [None, flow]


def write_frames(folder, T, h, w):
    from PIL import Image
    os.makedirs(folder, exist_ok=True)
    for i in range(T):
        Image.fromarray(np.full((h, w, 3), i, dtype=np.uint8)).save(os.path.join(folder, f"{i:05d}.png"))
    return folder


def load_reference(model):
    ref_harness.load()
    weights = types.SimpleNamespace(DEFAULT=types.SimpleNamespace(transforms=lambda: (lambda a, b: (a, b))))
    models = types.ModuleType("torchvision.models")
    optical_flow = types.ModuleType("torchvision.models.optical_flow")
    optical_flow.Raft_Large_Weights = weights
    optical_flow.raft_large = lambda weights=None, progress=False: model
    models.optical_flow = optical_flow
    sys.modules["torchvision.models"] = models
    sys.modules["torchvision.models.optical_flow"] = optical_flow
    import cv2

    def resize(img, dsize, interpolation=None):
        assert (img.shape[1], img.shape[0]) == tuple(dsize), "only the identity resize is stood in for"
        return np.array(img, copy=True)

    cv2.resize, cv2.INTER_LINEAR = resize, 1
    import preprocessing.extract_trajectories as ET
    ET.device = "cpu"
    ET.tzip = lambda *its, **k: zip(*its)
    ET.tqdm = lambda it, **k: it
    return ET


def run_reference(ET, model, case, min_len, direct):
    """(trajectories [N, T, 2] float32, masks [T, h, w] bool) of the reference script on one case"""
    model.case, kept = case, {}
    inner_masks, inner_direct = ET.get_flows_with_masks, ET.compute_direct_flows_for_start_frame

    def masks_spy(*a, **k):
        out = inner_masks(*a, **k)
        kept["masks"] = out[0]
        return out

    def direct_mode(*a, **k):
        model.direct = True
        try:
            return inner_direct(*a, **k)
        finally:
            model.direct = False

    cuda = torch.Tensor.cuda
    torch.Tensor.cuda = lambda self, *a, **k: self
    ET.get_flows_with_masks, ET.compute_direct_flows_for_start_frame = masks_spy, direct_mode
    try:
        with tempfile.TemporaryDirectory() as tmp:
            frames = write_frames(os.path.join(tmp, "frames"), case["T"], case["h"], case["w"])
            out_path = os.path.join(tmp, "out", "traj.pt")
            ET.save_trajectories(types.SimpleNamespace(
                frames_path=frames, output_path=out_path, infer_res_size=None, threshold=D.THRESHOLD,
                min_trajectory_length=min_len, filter_using_direct_flow=direct,
                direct_flow_threshold=D.DIRECT_THRESHOLD if direct else None))
            traj = torch.load(out_path)
    finally:
        torch.Tensor.cuda = cuda
        ET.get_flows_with_masks, ET.compute_direct_flows_for_start_frame = inner_masks, inner_direct
    assert traj.dtype == torch.float32 and traj.shape[1:] == (case["T"], 2)
    masks = kept["masks"].reshape(case["T"] + 1, case["h"], case["w"])[:case["T"]]   # the script allocates one frame too many
    return traj, masks


def key(name, direct):
    return f"{name}_{'direct' if direct else 'plain'}"


def main():
    model = FlowLookup()
    ET = load_reference(model)
    out = {}
    for name, (make, min_len) in D.GOLDEN_CASES.items():
        case = make()
        out[f"digest_{name}"] = np.array(D.case_digest(case))
        rows = {}
        for direct in (False, True):
            traj, masks = run_reference(ET, model, case, min_len, direct)
            rows[direct] = traj
            out[f"traj_{key(name, direct)}"] = traj.numpy()
            out[f"masks_{key(name, direct)}"] = masks.numpy()
            ok = ~traj.isnan().any(-1)
            starts = sorted(set(ok.float().argmax(1).tolist()))
            print(f"{key(name, direct)}: {tuple(traj.shape)} starts {starts} lengths {sorted(set(ok.sum(1).tolist()))}")
            # starts occur at every eligible frame
            assert starts == list(range(case["T"] - (min_len - 1))), starts
            args = (case["fflow"], case["bflow"], D.THRESHOLD, min_len) + \
                ((lambda s: case["direct"][s], D.DIRECT_THRESHOLD) if direct else (None, None))
            if name.startswith("lattice"):
                assert R.same_bits(R.chain_trajectories(*args), traj), "fp32 restatement != reference on the lattice"
            else:
                margin = R.Margin()
                wide = R.chain_trajectories(*args, dtype=torch.float64, margin=margin)
                same, dev = R.same_pattern_within(wide, traj, float("inf"))
                assert same, "reference and float64 restatement keep different rows: pick another seed in traj_data.SMOOTH"
                out["ref_dev"] = np.array(max(dev, float(out.get("ref_dev", 0.0))))
                out["margin"] = np.array(min(margin.value, float(out.get("margin", np.inf))))
                print(f"  reference vs float64 restatement: max deviation {dev:.3g} px, smallest decision margin {margin.value:.3g}")
        # the direct filter changes the row set
        a, b = rows[False], rows[True]
        changed = a.shape[0] != b.shape[0] or int(((a != b) & ~(a.isnan() & b.isnan())).any(-1).any(-1).sum())
        differing = abs(a.shape[0] - b.shape[0]) if a.shape[0] != b.shape[0] else changed
        assert changed and (name != "smooth" or differing >= 20), (name, differing)
    np.savez_compressed(OUT, **out)
    size = os.path.getsize(OUT)
    print(f"wrote {OUT} ({size / 1024:.0f} KiB), {model.calls} stand-in flow calls")
    assert size < 1 << 20


if __name__ == "__main__":
    main()
