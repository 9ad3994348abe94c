"""Inputs of the track-video golden (tests/golden/viz.npz, make_golden_viz.py): a synthetic pan with mild perspective, seeded and
bit-identical everywhere (numpy's PCG64 streams and float64 arithmetic only).

  T = 6 frames of 80 x 50; 40 background tracks that follow the camera (15 % of them gross outliers with a motion of their own;
  entries that leave the frame and a few random ones are NaN = occluded, as bg_trajectories.pt stores them); 9 foreground points
  with their own motion, some occluded, some leaving the frame.
"""
import numpy as np

T, H, W = 6, 50, 80
N_BG, N_FG = 40, 9
OUTLIER_FRAC = 0.15
NP_RANDOM_SEED = 1234          # np.random.seed(...) before get_homographies_wrt_frame
POINT_SIZE, LINEWIDTH = 40, 1.5


def camera(t):
    """3 x 3 map from the canonical plane to frame t: a pan to the right and slightly down, a small zoom, mild perspective."""
    s = 1.0 + 0.01 * t
    return np.array([[s, 0.004 * t, -3.1 * t + 6.0],
                     [-0.003 * t, s, -1.3 * t + 2.0],
                     [4e-5 * t, -3e-5 * t, 1.0]])


def project(h, p):
    q = np.concatenate([p, np.ones((len(p), 1))], axis=1) @ h.T
    return q[:, :2] / q[:, 2:]


def background():
    """(tracks [N_BG, T, 2] float32 with NaN where occluded, outlier flags [N_BG])."""
    rng = np.random.default_rng(7)
    base = rng.uniform([2.0, 2.0], [W + 12.0, H + 4.0], size=(N_BG, 2))
    tracks = np.stack([project(camera(t), base) for t in range(T)], axis=1)
    tracks += rng.normal(0.0, 0.05, size=tracks.shape)
    outlier = np.zeros(N_BG, dtype=bool)
    outlier[rng.choice(N_BG, int(round(OUTLIER_FRAC * N_BG)), replace=False)] = True
    drift = rng.uniform(-9.0, 9.0, size=(N_BG, 1, 2)) * np.arange(T)[None, :, None] + rng.uniform(-6.0, 6.0, size=(N_BG, T, 2))
    tracks = np.where(outlier[:, None, None], tracks + drift, tracks)
    gone = (tracks[..., 0] < 0) | (tracks[..., 0] > W - 1) | (tracks[..., 1] < 0) | (tracks[..., 1] > H - 1)
    gone |= rng.random((N_BG, T)) < 0.06
    tracks[gone] = np.nan
    return tracks.astype(np.float32), outlier


def foreground():
    """(points [N_FG, T, 2] float32, occluded [N_FG, T] int32): some points leave the frame on the right / top / left."""
    rng = np.random.default_rng(11)
    start = rng.uniform([12.0, 10.0], [W - 12.0, H - 10.0], size=(N_FG, 2))
    vel = rng.uniform(-4.0, 4.0, size=(N_FG, 2))
    vel[0], start[0] = [9.3, 0.7], [52.3, 20.6]          # leaves on the right
    vel[1], start[1] = [-1.1, -6.2], [30.4, 17.7]        # leaves at the top
    vel[2], start[2] = [-7.9, 2.3], [21.2, 30.9]         # leaves on the left
    pts = start[:, None] + vel[:, None] * np.arange(T)[None, :, None] + rng.normal(0.0, 0.4, size=(N_FG, T, 2))
    occ = (rng.random((N_FG, T)) < 0.15).astype(np.int32)
    occ[4, 2:4] = 1
    return pts.astype(np.float32), occ


def video():
    """[T, H, W, 3] uint8: a smooth pattern that moves with the camera plus seeded noise."""
    rng = np.random.default_rng(13)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    out = []
    for t in range(T):
        u, v = x + 3.1 * t, y + 1.3 * t
        img = np.stack([127 + 90 * np.sin(u / 7.0) * np.cos(v / 5.0), 127 + 90 * np.cos(u / 11.0 + v / 9.0), 60 + 1.5 * u + 0.5 * v],
                       axis=-1)
        out.append(np.clip(img + rng.normal(0, 6, size=img.shape), 0, 255))
    return np.stack(out).astype(np.uint8)


def write_data_folder(root):
    """The scene as a data folder in the layout of utils.add_config_paths: video/ and masks/ PNGs, grid_trajectories/,
    grid_occlusions/, of_trajectories/bg_trajectories.pt.  The mask is foreground everywhere but the top-left corner."""
    import os

    import torch
    from PIL import Image
    for sub in ("video", "masks", "grid_trajectories", "grid_occlusions", "of_trajectories"):
        os.makedirs(os.path.join(root, sub), exist_ok=True)
    for t, frame in enumerate(video()):
        Image.fromarray(frame).save(os.path.join(root, "video", f"{t:05d}.png"))
    mask = np.full((H, W), 255, dtype=np.uint8)
    mask[:6, :6] = 0
    for t in range(T):
        Image.fromarray(mask).save(os.path.join(root, "masks", f"{t:05d}.png"))
    pts, occ = foreground()
    np.save(os.path.join(root, "grid_trajectories", "grid_trajectories.npy"), pts)
    np.save(os.path.join(root, "grid_occlusions", "grid_occlusions.npy"), occ.astype(bool))
    torch.save(torch.from_numpy(background()[0]), os.path.join(root, "of_trajectories", "bg_trajectories.pt"))
    return root
