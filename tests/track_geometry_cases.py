"""Case table shared by tests/test_gpu_track_geometry.py (the kernels) and tests/test_track_geometry_cases.py (the premises):
token grids other than the benchmark's 67 x 121 at which the matrix-core tracker (csrc/track_mfma.hip) has geometry-dependent
behaviour -- row padding to 128 cells, the 13-bit position tag of corr_peaks, windows clamped at (or larger than) the map, the
key range rounded up from ph, the LDS size of head16.

Every case: patch 14, stride 7, T = 2, features synth_features(T, C, ph, pw, seed=70), head synth_head_weights(3), M = 300 sources
(not a multiple of 256: the last workgroup is ragged).  The first eight sources are the exact features of the four corner cells
and the four edge midpoints of their target frame (arg-max on the border: clamped windows); the other 292 are bilinear samples at
random points of random source frames, tracked into random target frames (generator seed 5)."""
import torch

from dino_tracker_amd import synth
from oracle import ref_algo as A

PATCH, STRIDE, T, M, FEAT_SEED, SRC_SEED, HEAD_SEED = 14, 7, 2, 300, 70, 5, 3
TABLE_ROWS = 40
TAG_LIMIT_CELLS = 16384   # ph * pw_pad(pw) up to which corr_peaks' position tag holds every step (restated from the source in the CPU file)

PEAKS, TILED = "corr_peaks", "corr16_peaks + select"

# (video H, video W, ph, pw, candidate kernel at C = 384 / 768 / 1024, feature widths, why)
GRIDS = [
    (854, 476, 121, 67, PEAKS, (384,), "portrait; 61 padding cells per row"),
    (256, 256, 35, 35, PEAKS, (384, 768, 1024), "TAP-Vid raster; 93 padding cells per row"),
    (98, 126, 13, 17, PEAKS, (384,), "ph < 15: window taller than the map"),
    (56, 70, 7, 9, PEAKS, (384,), "both sides below the window"),
    (105, 910, 14, 129, PEAKS, (384, 64), "pw just over one tile: pw_pad = 256, 127 padding cells per row"),
    (455, 910, 64, 129, PEAKS, (384, 768, 1024), "ph * pw_pad = 16 384: last admitted step, tag all ones"),
    (903, 903, 128, 128, PEAKS, (384,), "16 384 again, no padding cell at all"),
    (462, 910, 65, 129, TILED, (384, 768, 1024), "one row past the limit"),
    (720, 1280, 101, 181, TILED, (384,), "the common 720p size"),
]


class Case:
    def __init__(self, H, W, ph, pw, C, kernel, why):
        self.H, self.W, self.ph, self.pw, self.C, self.why = H, W, ph, pw, C, why
        # C = 64 is below the widths corr_peaks serves: the generic pair whatever the grid
        self.kernel = kernel if C in (384, 768, 1024) else TILED
        self.id = f"{ph}x{pw}-C{C}"

    def __repr__(self):
        return self.id


CASES = [Case(H, W, ph, pw, C, kernel, why) for (H, W, ph, pw, kernel, widths, why) in GRIDS for C in widths]

# The exact fp32 path (TRACK_EXACT, and tier 3 of TRACK_MFMA) keeps a map's logits and a ring of hidden rows in LDS; head_exact_kernel
# has a form with the map in LDS too and a large-grid form without.  (ph, pw, what is expected): the last grid of the first form,
# the first and the last of the second, the first that is refused -- at pw = 100, C = 32, T = 1.
EXACT_FORM_GRIDS = [(140, 100, "map in LDS"), (141, 100, "large grid"), (345, 100, "large grid"), (346, 100, "refused")]


def exact_head_lds_floats(ph, pw, large, hr=6, hr_large=2, hidden=16):
    """LDS demand of head_exact_kernel in floats (exact_head_lds in track_exact.hip, restated)."""
    hwp = (ph * pw + 3) // 4 * 4
    return (1 if large else 2) * hwp + hidden * ((hr_large if large else hr) + 2) * pw + 16


def exact_form(ph, pw, lds_bytes=160 * 1024, **kw):
    if 4 * exact_head_lds_floats(ph, pw, False, **kw) <= lds_bytes:
        return "map in LDS"
    return "large grid" if 4 * exact_head_lds_floats(ph, pw, True, **kw) <= lds_bytes else "refused"


def pw_pad(pw, cn=128):
    return (pw + cn - 1) // cn * cn


def border_cells(ph, pw):
    """(row, col) of the four corners and the four edge midpoints."""
    return [(0, 0), (0, pw - 1), (ph - 1, 0), (ph - 1, pw - 1),
            (0, pw // 2), (ph - 1, pw // 2), (ph // 2, 0), (ph // 2, pw - 1)]


def features(case):
    return synth.synth_features(T, case.C, case.ph, case.pw, seed=FEAT_SEED)


def head_weights():
    return synth.synth_head_weights(HEAD_SEED)


def sources(case, feats):
    """(src [M, C], tgt [M]): the eight border sources first (target frame i % T), then 292 random ones."""
    cells = border_cells(case.ph, case.pw)
    n = M - len(cells)
    g = torch.Generator().manual_seed(SRC_SEED)
    pts = torch.rand(n, 2, generator=g) * torch.tensor([case.W - 1.0, case.H - 1.0])
    ts = torch.randint(0, T, (n,), generator=g)
    tg = torch.randint(0, T, (n,), generator=g)
    rnd = A.sample_bilinear(feats, pts, ts, case.H, case.W, PATCH, STRIDE)
    btgt = torch.arange(len(cells)) % T
    bsrc = torch.stack([feats[int(t), :, r, c] for t, (r, c) in zip(btgt, cells)])
    return torch.cat([bsrc, rnd]).contiguous(), torch.cat([btgt, tg])


def row_table(src, tgt):
    """The row-table form: (table [40, C], src_row [M]).  The table holds the first 40 sources (the border ones among them); every
    row is referenced 7 or 8 times, in shuffled order, each time tracked into the target frame of that position of `tgt`."""
    g = torch.Generator().manual_seed(SRC_SEED + 1)
    src_row = (torch.arange(M) % TABLE_ROWS)[torch.randperm(M, generator=g)]
    return src[:TABLE_ROWS].contiguous(), src_row


def cosine64(src, feats, tgt):
    """Float64 cosine maps [M, ph * pw] of every source against its target frame (raw: no ReLU)."""
    t, c, h, w = feats.shape
    out = torch.empty(src.shape[0], h * w, dtype=torch.float64)
    s = src.double()
    for f in range(t):
        sel = torch.nonzero(tgt == f)[:, 0]
        fr = feats[f].double().reshape(c, h * w)
        out[sel] = (s[sel] @ fr) / (s[sel].norm(dim=1)[:, None] * fr.norm(dim=0)[None]).clamp(min=A.EPS)
    return out
