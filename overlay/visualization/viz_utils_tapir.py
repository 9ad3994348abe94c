"""Drop-in for the reference's visualization/viz_utils_tapir.py: the functions visualize_rainbow.py calls, rendered on the device
(dino_tracker_amd/visualize.py, docs/RENDER.md) instead of through matplotlib."""
from dino_tracker_amd.visualize import (compute_canonical_points, compute_inliers, estimate_homography,  # noqa: F401
                                        get_homographies_wrt_frame, maybe_ransac_homography, plot_tracks_tails, plot_tracks_v2,
                                        ransac_homography)
