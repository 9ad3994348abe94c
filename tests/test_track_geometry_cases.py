"""CPU: the premises of tests/test_gpu_track_geometry.py, so that they cannot rot.  For every case of tests/track_geometry_cases.py:
the token grid is the stated one; ph * pw_pad is on the stated side of the position-tag limit of corr_peaks (the launcher's
arithmetic restated, its constants parsed from track_mfma.hip); on the case's sources -- the direct form and the row-table form --
the oracle alone produces nothing that must leave the fast tier (no zero-mass fallback, at most KC cells within EPS_C of the
maximum, a positive maximum), the float64 arg-max is unambiguous (top-two gap above 1e-5, fp32 and float64 agree) and the eight
border sources peak at their border cells; the table form and the direct form are the same to the oracle.

All 300 sources of every case, the two largest grids included: the maps are one matrix product per target frame, as A.track forms
them, and the head runs on 64 maps at a time (the whole file takes well under a minute)."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import track_geometry_cases as G
from oracle import ref_algo as A

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "dino_tracker_amd", "csrc")
with open(os.path.join(CSRC, "track_mfma.hip")) as _fh:
    SRC = _fh.read()


def _const(pattern, conv=int):
    return conv(re.search(pattern, SRC).group(1))


PK_IDX_BITS = _const(r"constexpr int PK_IDX_BITS = (\d+);")
CN = _const(r"constexpr int CM = \d+, CN = (\d+), CK = \d+;")
KC = _const(r"constexpr int KC = (\d+);")
EPS_C = _const(r"constexpr float EPS_C = ([0-9.eE+-]+)f;", float)
PK_CB = _const(r"constexpr int PK_CB = (\d+);")
RD = _const(r"constexpr int RD = (\d+);")
assert "constexpr int WX = 2 * RD + 5;" in SRC
WX = 2 * RD + 5


def test_the_case_table_is_the_one_the_issue_states():
    assert (PK_IDX_BITS, CN, KC, EPS_C, PK_CB, WX) == (13, 128, 10, 3e-3, 1, 15)
    assert len(G.GRIDS) == 9 and len(G.CASES) == 16 and G.M == 300 and G.M % 256 != 0 and G.TABLE_ROWS < G.M
    grids = {(ph, pw): k for (_, _, ph, pw, k, _, _) in G.GRIDS}
    assert grids == {(121, 67): G.PEAKS, (35, 35): G.PEAKS, (13, 17): G.PEAKS, (7, 9): G.PEAKS, (14, 129): G.PEAKS,
                     (64, 129): G.PEAKS, (128, 128): G.PEAKS, (65, 129): G.TILED, (101, 181): G.TILED}
    widths = {(ph, pw): w for (_, _, ph, pw, _, w, _) in G.GRIDS}
    for grid, w in widths.items():
        assert 384 in w
        assert set(w) == ({384, 768, 1024} if grid in ((35, 35), (64, 129), (65, 129)) else {384, 64} if grid == (14, 129) else {384})
    # what each grid is in the table for
    assert G.pw_pad(67) - 67 == 61 and G.pw_pad(35) - 35 == 93 and G.pw_pad(129) == 256 and G.pw_pad(129) - 129 == 127 and G.pw_pad(128) == 128
    assert 13 < WX and 7 < WX and 9 < WX and 17 > WX
    assert 64 * G.pw_pad(129) == 128 * G.pw_pad(128) == G.TAG_LIMIT_CELLS and 65 * G.pw_pad(129) == G.TAG_LIMIT_CELLS + 256


@pytest.mark.parametrize("case", G.CASES, ids=repr)
def test_grid_and_side_of_the_tag_limit(case):
    assert A.feature_grid(case.H, case.W, G.PATCH, G.STRIDE) == (case.ph, case.pw)
    assert G.pw_pad(case.pw, CN) == (case.pw + CN - 1) // CN * CN
    hwp = case.ph * G.pw_pad(case.pw, CN)
    # mfma_phase's `peaks_shape`, restated: one step is 32 * PK_CB cells, the tag holds step << 4 | register (one more bit with two cell blocks)
    cells = 32 * PK_CB
    steps = hwp // cells
    admitted = (steps <= 1 << (PK_IDX_BITS - (5 if PK_CB > 1 else 4)) and hwp % cells == 0 and G.pw_pad(case.pw, CN) % cells == 0
                and G.T * hwp * case.C * 2 < 1 << 32)
    assert (1 << (PK_IDX_BITS - 4)) * cells == G.TAG_LIMIT_CELLS
    assert admitted == (hwp <= G.TAG_LIMIT_CELLS)
    served = case.C == 384 or case.C in (768, 1024)
    assert (G.PEAKS if admitted and served else G.TILED) == case.kernel
    if (case.ph, case.pw) in ((64, 129), (128, 128)):
        assert hwp == G.TAG_LIMIT_CELLS and ((steps - 1) << 4 | 15) == (1 << PK_IDX_BITS) - 1   # the last step's tag is all ones
    if (case.ph, case.pw) == (65, 129):
        assert hwp - G.TAG_LIMIT_CELLS == G.pw_pad(case.pw, CN)                                   # exactly one row past it


def test_forms_of_the_exact_head_and_its_grid_limit():
    """The grids at which the exact path changes form or refuses (EXACT_FORM_GRIDS) are on the stated sides, by the launcher's
    arithmetic with the constants of track_exact.hip; of the case table only the two largest grids take the large-grid form, and
    none is refused."""
    with open(os.path.join(CSRC, "track_exact.hip")) as fh:
        ex = fh.read()
    with open(os.path.join(os.path.dirname(os.path.dirname(CSRC)), "include", "dtk.h")) as fh:
        hc = fh.read()
    kw = dict(hr=int(re.search(r"constexpr int HR = (\d+);", ex).group(1)),
              hr_large=int(re.search(r"constexpr int HR_LARGE = (\d+);", ex).group(1)),
              hidden=int(re.search(r"#define DTK_HEAD_HIDDEN (\d+)", hc).group(1)))
    assert "constexpr size_t EXACT_LDS_MAX = 160 * 1024;" in ex
    assert "(large ? 1 : 2) * HWp + DTK_HEAD_HIDDEN * ((large ? HR_LARGE : HR) + 2) * g->pw + 16" in ex
    assert kw == dict(hr=6, hr_large=2, hidden=16)
    for ph, pw, want in G.EXACT_FORM_GRIDS:
        assert G.exact_form(ph, pw, **kw) == want, (ph, pw)
    forms = {(c.ph, c.pw): G.exact_form(c.ph, c.pw, **kw) for c in G.CASES}
    assert {g for g, f in forms.items() if f == "large grid"} == {(128, 128), (101, 181)}
    assert "refused" not in forms.values()
    assert G.exact_form(153, 273, **kw) == "refused"   # 1080 x 1920: documented in include/dtk.h


@pytest.fixture(scope="module", params=G.CASES, ids=repr)
def premises(request):
    case = request.param
    feats = G.features(case)
    src, tgt = G.sources(case, feats)
    table, src_row = G.row_table(src, tgt)
    return case, feats, src, tgt, table, src_row


def _maps32(src, feats, tgt):
    """The fp32 cosine maps [M, ph * pw] as A.track forms them: one product per target frame."""
    t, c, h, w = feats.shape
    out = torch.empty(src.shape[0], h * w)
    for f in range(t):
        sel = torch.nonzero(tgt == f)[:, 0]
        fr = feats[f].reshape(c, h * w)
        out[sel] = (src[sel] @ fr) / (src[sel].norm(dim=1)[:, None] * fr.norm(dim=0)[None]).clamp(min=A.EPS)
    return out


def _map_premises(case, feats, src, tgt, what):
    cos = G.cosine64(src, feats, tgt)
    top2 = cos.topk(2, dim=1)
    best, gap = top2.values[:, 0], top2.values[:, 0] - top2.values[:, 1]
    in_band = (cos >= best[:, None] - EPS_C).sum(dim=1)
    assert float(best.min()) > 2 * EPS_C, (what, float(best.min()))                  # positive, and beyond the single-candidate threshold
    assert int(in_band.max()) <= KC, (what, int(in_band.max()))                        # no candidate list overflows
    assert float(gap.min()) > 1e-5, (what, float(gap.min()), int(gap.argmin()))        # the arg-max is not an fp32 near-tie
    assert torch.equal(_maps32(src, feats, tgt).argmax(dim=1), top2.indices[:, 0]), what   # fp32 and float64 agree for every source
    return top2.indices[:, 0], float(gap.min())


def test_maps_leave_nothing_for_the_slow_tiers(premises):
    case, feats, src, tgt, table, src_row = premises
    k, gap = _map_premises(case, feats, src, tgt, "direct")
    _, gap_t = _map_premises(case, feats, table[src_row], tgt, "table")
    want = torch.tensor([r * case.pw + c for r, c in G.border_cells(case.ph, case.pw)])
    assert torch.equal(k[:8], want), (k[:8], want)
    # the table form tracks border rows into both frames; into their own frame they peak at their own cell
    own = torch.nonzero((src_row < 8) & (tgt == src_row % G.T))[:, 0]
    assert own.numel() >= 8
    kt = G.cosine64(table[src_row[own]], feats, tgt[own]).argmax(dim=1)
    assert torch.equal(kt, want[src_row[own]])
    print(f"{case}: float64 top-two gap >= {gap:.2e} (direct), {gap_t:.2e} (table)")


def test_no_fallback_and_table_form_equals_direct_form(premises):
    case, feats, src, tgt, table, src_row = premises
    head = G.head_weights()
    for s, what in ((src, "direct"), (table[src_row], "table")):
        x = F.relu(_maps32(s, feats, tgt)).reshape(G.M, case.ph, case.pw)
        for i in range(0, G.M, 64):
            _, _, _, fb = A.tracker_head(x[i:i + 64], head, case.H, case.W, G.PATCH, G.STRIDE, return_aux=True)
            assert int(fb.sum()) == 0, (what, i)
    tabled = A.track(table, feats, tgt, head, case.H, case.W, G.PATCH, G.STRIDE, src_row=src_row)
    gathered = A.track(table[src_row].contiguous(), feats, tgt, head, case.H, case.W, G.PATCH, G.STRIDE)
    assert torch.isfinite(tabled).all() and torch.equal(gathered, tabled)
