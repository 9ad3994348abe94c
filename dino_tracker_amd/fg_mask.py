"""PCA foreground masks on the device: preprocessing/create_fg_mask.py without the reference checkout.

The reference min-max normalises the first principal component of the L2-normalised DINO features of the whole video and calls
a token foreground where it is below a threshold.  It gets the component from `torch.pca_lowrank(features, q=3, niter=20)` --
about forty passes over the [T h w, C] matrix.  Here the component comes from the exact PCA:

* `ops.pca_moments`  -- mean and centred Gram matrix of the normalised rows, one MFMA kernel over the volume (dtk_pca_moments),
* the eigenvectors of that C x C matrix: it is at most 4 MB, so it is copied to the host and `torch.linalg.eigh` runs there in
  float64.  That is ONE stream synchronisation in a preprocessing step; there is no device eigensolver,
* `ops.pca_project`  -- the rows (uncentred, as the reference projects them) on the top q eigenvectors, with min / max,
* `ops.fg_mask`      -- threshold and nearest upsampling to the image size.

Sign.  An eigenvector is defined up to its sign and the reference takes whatever its randomised SVD returns: on a video whose
foreground is a small blob it can label 77 % of the tokens foreground -- the inverted mask.  The reference has no rule, so this
module has a deterministic one.  The raw sign makes the largest-magnitude entry of every eigenvector positive (lowest index on
ties).  Then `orient`:
  "positive"  stops there;
  "border"    (default) flips component 0 when the mean normalised colour over the outermost ring of the token grid (rows 0 and
              h - 1, columns 0 and w - 1, all frames) is below the mean over all tokens, so that the border lands on the background
              side of the threshold; equal means do not flip.
`invert=True` flips after either: it is the override for a video whose subject fills the border.

Command line (the reference's flags, plus --orient / --invert; lossless PNGs instead of the reference's JPEGs, whose compression
noise ends up in a mask that is later tested with `> 0`; both load_masks implementations glob *.png):
    python -m dino_tracker_amd.fg_mask --dino-embed-video-path P --h H --w W --mask-path M [--fg_mask_threshold 0.4] [--q 3]
                                       [--orient border|positive] [--invert]
"""
from __future__ import annotations

import argparse
import os
from typing import Optional, Tuple

import torch

from . import ops

ORIENTATIONS = ("border", "positive")


def principal_components(cov: torch.Tensor, q: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(V [q, C] float64, eigenvalues [q] descending) of a symmetric matrix, on the host in float64 (one synchronisation when
    `cov` lives on the device); raw sign: the largest-magnitude entry of every row is positive, the lowest index on ties."""
    w, v = torch.linalg.eigh(cov.detach().to(device="cpu", dtype=torch.float64))
    V = v[:, -q:].flip(1).T.contiguous()
    lead = V.gather(1, V.abs().argmax(dim=1, keepdim=True))   # argmax: the first of equal maxima
    V = torch.where(lead < 0, -V, V)
    return V, w[-q:].flip(0)


def border_flip(c0: torch.Tensor) -> bool:
    """c0 [T, h, w]: min-max normalised component 0.  True when the outermost ring of the grid is, on average, below all tokens."""
    ring = torch.zeros(c0.shape[1:], dtype=torch.bool, device=c0.device)
    ring[0, :] = ring[-1, :] = True
    ring[:, 0] = ring[:, -1] = True
    c0 = c0.double()
    return bool(c0[:, ring].mean() < c0.mean())


@torch.no_grad()
def get_fg_mask_from_pca(feature_map: torch.Tensor, img_size, q: int = 3, interpolation: str = "nearest", normalize: bool = True,
                         fg_mask_threshold: float = 0.4, *, orient: str = "border", invert: bool = False,
                         return_details: bool = False):
    """create_fg_mask.get_fg_mask_from_pca on device features [T, h, w, C] (or [h, w, C]), C = 384 / 768 / 1024 ->
    [T, H, W] float32 numpy array of 0 / 1, like the reference.  There is no CPU path.

    The component is the exact first principal component (see the module docstring): the eigen-decomposition runs on the host in
    float64 and costs one synchronisation.  The reference's sign is unspecified; `orient` ("border" | "positive") fixes it and
    `invert=True` is the override.  With `return_details` the result is (array, details): details["mask"] the device uint8
    [T, H, W] mask (0 / 255), ["token_mask"] [T, h, w], ["colors"] the min-max normalised colours [T, h, w, q] (component 0 as
    thresholded, i.e. one minus it when flipped), ["flipped"], ["eigenvalues"] (the top q)."""
    if interpolation != "nearest":
        raise NotImplementedError(f"interpolation={interpolation!r}: the device masks are nearest-upsampled, like the reference's run()")
    if orient not in ORIENTATIONS:
        raise ValueError(f"orient {orient!r}: one of {ORIENTATIONS}")
    if feature_map.dim() == 3:
        feature_map = feature_map[None]
    if feature_map.dim() != 4:
        raise ValueError(f"feature_map must be [T, h, w, C] or [h, w, C], got {tuple(feature_map.shape)}")
    T, h, w, C = feature_map.shape
    x = feature_map.to(torch.float32).contiguous()
    _, cov = ops.pca_moments(x, normalize=normalize)
    V, evals = principal_components(cov, q)
    colors, minmax = ops.pca_project(x, V.to(device=x.device, dtype=torch.float32).contiguous(), normalize=normalize)
    mn, mx = minmax[:q], minmax[ops.PCA_MAX_Q:ops.PCA_MAX_Q + q]
    flip = False
    if orient == "border":
        flip = border_flip(((colors[:, 0] - mn[0]) / (mx[0] - mn[0])).reshape(T, h, w))
    flip ^= bool(invert)
    mask, tok = ops.fg_mask(colors, minmax, (T, h, w), img_size, fg_mask_threshold, comp=0, flip=flip)
    out = (mask > 0).to(torch.float32).cpu().numpy()
    if not return_details:
        return out
    norm = (colors - mn) / (mx - mn)
    if flip:
        norm[:, 0] = 1.0 - norm[:, 0]
    return out, {"mask": mask, "token_mask": tok, "colors": norm.reshape(T, h, w, q), "flipped": flip, "eigenvalues": evals}


@torch.no_grad()
def fg_masks_from_features(features: torch.Tensor, img_size, grid: Optional[Tuple[int, int]] = None, device="cuda:0", **kwargs):
    """The masks of a feature file [T, C, h, w] (packed through ops.pack_features) or of an already token-major [T, h w, C] volume
    with grid=(h, w); keywords as get_fg_mask_from_pca."""
    if features.dim() == 4:
        T, C, h, w = features.shape
        packed, _ = ops.pack_features(features.to(device=device, dtype=torch.float32).contiguous())
    elif features.dim() == 3 and grid is not None:
        h, w = grid
        T, HW, C = features.shape
        if HW != h * w:
            raise ValueError(f"features {tuple(features.shape)} do not fit the grid {h}x{w}")
        packed = features.to(device=device, dtype=torch.float32).contiguous()
    else:
        raise ValueError("features must be [T, C, h, w], or [T, h w, C] with grid=(h, w)")
    return get_fg_mask_from_pca(packed.view(T, h, w, C), img_size, **kwargs)


@torch.no_grad()
def fg_masks_from_video(video: torch.Tensor, model_name: str = "dinov2_vitl14", layer: int = 23, stride: int = 7, img_size=None,
                        device="cuda:0", extractor=None, frame_batch: int = 8, extractor_kwargs=None, **kwargs):
    """The masks of a video [T, 3, H, W] in [0, 1]: the DINO features of `layer` (config/preprocessing.yaml: dinov2_vitl14,
    layer 23, stride 7) straight from the device encoder -- they never leave the device -- then get_fg_mask_from_pca.
    `img_size` defaults to the video's."""
    from .extractor import VitExtractor
    ex = extractor if extractor is not None else VitExtractor(model_name=model_name, stride=stride, device=device,
                                                              **(extractor_kwargs or {}))
    T, _, H, W = video.shape
    h, w = ex.get_height_patch_num(video[[0]].shape), ex.get_width_patch_num(video[[0]].shape)
    feats = None
    for t0 in range(0, T, frame_batch):
        f = ex.encode(video[t0:t0 + frame_batch], layer=layer, normalize=True, want="feat")
        if feats is None:
            feats = torch.empty((T, h * w, f.shape[-1]), dtype=torch.float32, device=f.device)
        feats[t0:t0 + f.shape[0]] = f
    return get_fg_mask_from_pca(feats.view(T, h, w, -1), (H, W) if img_size is None else img_size, **kwargs)


# What DTK_PNG_ENCODE=auto selects.  The device encoder is opt-in until a change flips this on the strength of
# docs/MEASUREMENTS.md "PNG encode" (the project's bar: not slower than the host path beyond the host path's own spread).
PNG_AUTO_USES_DEVICE = False


def png_encode_on_device() -> bool:
    """DTK_PNG_ENCODE = host | device | auto (the default): `host` writes masks through Pillow, `device` through the device PNG
    encoder (png_out.py), `auto` does what PNG_AUTO_USES_DEVICE says.  Anything else raises."""
    mode = os.environ.get("DTK_PNG_ENCODE", "auto")
    if mode not in ("auto", "device", "host"):
        raise ValueError(f"DTK_PNG_ENCODE must be auto, device or host, got {mode!r}")
    return mode == "device" or (mode == "auto" and PNG_AUTO_USES_DEVICE)


def save_masks(mask: torch.Tensor, mask_path: str) -> str:
    """mask [T, H, W] uint8 -> mask_path/{idx:05d}.png (the names of data_utils.save_video_frames, lossless).  Pillow writes them,
    or the device encoder where DTK_PNG_ENCODE selects it (png_encode_on_device): the same pixels either way."""
    if png_encode_on_device():
        from . import png_out
        return png_out.write_png_frames(mask if mask.is_cuda else mask.numpy(), mask_path)
    from PIL import Image
    os.makedirs(mask_path, exist_ok=True)
    for idx, m in enumerate(mask.cpu().numpy()):
        Image.fromarray(m).save(os.path.join(mask_path, f"{idx:05d}.png"))
    return mask_path


def run(dino_embed_video_path: str, h: int, w: int, mask_path: str, fg_mask_threshold: float = 0.4, q: int = 3,
        orient: str = "border", invert: bool = False, device="cuda:0") -> torch.Tensor:
    """create_fg_mask.run: the feature file T x C x h x w -> the mask frames; returns the device mask."""
    features = torch.load(dino_embed_video_path, map_location="cpu")
    _, details = fg_masks_from_features(features, (h, w), device=device, q=q, fg_mask_threshold=fg_mask_threshold, orient=orient,
                                        invert=invert, return_details=True)
    print(f"Saved fg. mask to {save_masks(details['mask'], mask_path)}")
    return details["mask"]


def main(argv=None):
    ap = argparse.ArgumentParser(prog="dino_tracker_amd.fg_mask")
    ap.add_argument("--dino-embed-video-path", type=str, required=True)
    ap.add_argument("--h", type=int, required=True)
    ap.add_argument("--w", type=int, required=True)
    ap.add_argument("--mask-path", type=str, required=True)
    ap.add_argument("--fg_mask_threshold", type=float, default=0.4)
    ap.add_argument("--q", type=int, default=3)
    ap.add_argument("--orient", choices=ORIENTATIONS, default="border")
    ap.add_argument("--invert", action="store_true")
    a = ap.parse_args(argv)
    run(a.dino_embed_video_path, a.h, a.w, a.mask_path, a.fg_mask_threshold, a.q, a.orient, a.invert)


if __name__ == "__main__":
    main()
