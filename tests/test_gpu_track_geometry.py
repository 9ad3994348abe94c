"""-m gpu: the tracker kernels at token grids other than the benchmark's 67 x 121 (cases: tests/track_geometry_cases.py, their
premises: tests/test_track_geometry_cases.py).  The production kernels of DTK_TRACK_MFMA -- corr_peaks / corr_peaks_wide,
refine_corr_dma, rescore, refine_head, the key sort -- and the tiled pair corr16_peaks + select at C = 384 / 768 / 1024 depend on
the grid through the row padding to 128 cells, the 13-bit position tag, the window clamps, the key range and the LDS size of
head16; every other GPU test of the tracker runs them at 67 x 121 only.

Per case, against oracle/ref_algo.py (A.track on the host, computed once per case): both methods and two round sizes, the
whole-map tier, the row-table form (src_row + emb_rows), which candidate kernel was launched, the tier counts, and
dtk_argmax_cells against the float64 cosine map.  Tolerances are the project's: 1e-3 px for positions, 2e-6 for a cosine.  One
end-to-end ModelInference.infer case at 35 x 35 (93 padding cells per row) and the grids at which the exact path changes form or
refuses close the file.  Measured errors and tier counts:
docs/PARITY.md, "Tracker kernels at other token grids"."""
import pytest
import torch

import track_geometry_cases as G
from dino_tracker_amd import ops, synth
from oracle import ref_algo as A

pytestmark = pytest.mark.gpu
PX_TOL = 1e-3
COS_TOL = 2e-6   # the bound of test_best_buddies
M = G.M


class _Case:
    pass


@pytest.fixture(scope="module", params=G.CASES, ids=repr)
def gc(request):
    """Inputs, host oracle and the two trackers of one case (built once, shared by the tests below; nothing here is modified
    by a test except the tracker options, which every test restores)."""
    from gpu_util import make_tracker
    case = request.param
    c = _Case()
    c.case = case
    c.feats = G.features(case)
    c.head = G.head_weights()
    c.src, c.tgt = G.sources(case, c.feats)
    c.table, c.src_row = G.row_table(c.src, c.tgt)
    c.ref = A.track(c.src, c.feats, c.tgt, c.head, case.H, case.W, G.PATCH, G.STRIDE)
    c.ref_table = A.track(c.table, c.feats, c.tgt, c.head, case.H, case.W, G.PATCH, G.STRIDE, src_row=c.src_row)
    cos = G.cosine64(c.src, c.feats, c.tgt)
    c.cos_max, c.cos_arg = cos.max(dim=1)
    video = torch.zeros(G.T, 3, case.H, case.W)   # only its size matters
    c.trk = {m: make_tracker(video, c.feats, c.head, method=m) for m in (ops.TRACK_EXACT, ops.TRACK_MFMA)}
    c.src_d, c.tgt_d = c.src.cuda().contiguous(), c.tgt.int().cuda()
    return c


def _run(c, method, emb=None, src_row=None, rounds=0, tier=ops.TIER_AUTO):
    """One dtk_track call through Tracker.track_sources into a NaN-filled buffer -> (positions on the host, stats)."""
    trk = c.trk[method]
    trk.track_round_sources, trk.track_tier, trk._workspace = rounds, tier, None
    try:
        out = torch.full((M, 2), float("nan"), device="cuda")
        trk.track_sources(trk.features(), c.src_d if emb is None else emb, src_row, c.tgt_d, None, out, M)
        torch.cuda.synchronize()
        return out.cpu(), dict(trk.last_track_stats)
    finally:
        trk.track_round_sources, trk.track_tier, trk._workspace = 0, ops.TIER_AUTO, None


def _check(c, out, ref, what):
    err = (out - ref).abs().max(dim=1).values
    print(f"{c.case} {what}: max err {float(err.max()):.2e} px (border sources {float(err[:8].max()):.2e})")
    assert torch.isfinite(out).all(), (what, torch.nonzero(~torch.isfinite(out).all(dim=1))[:, 0].tolist())
    assert err[:8].max() < PX_TOL, (what, "border sources (corners, edge midpoints)", err[:8].tolist())
    assert err.max() < PX_TOL, (what, int(err.argmax()), float(err.max()))
    return err


def test_methods_and_rounds(gc):
    """TRACK_EXACT, TRACK_MFMA in one round and in rounds of 256 (two rounds, the second ragged: 44 sources)."""
    out_e, _ = _run(gc, ops.TRACK_EXACT)
    _check(gc, out_e, gc.ref, "exact")
    out_1, st1 = _run(gc, ops.TRACK_MFMA)
    _check(gc, out_1, gc.ref, "mfma, one round")
    out_2, st2 = _run(gc, ops.TRACK_MFMA, rounds=256)
    _check(gc, out_2, gc.ref, "mfma, rounds of 256")
    assert st1["sources"] == M and st2["sources"] == M
    assert torch.equal(out_1, out_2)   # the round size is not visible in the results


def test_whole_map_tier(gc):
    """head16 at this grid's LDS size: (ph + 2) x (pw_pad + 16) halves."""
    out, st = _run(gc, ops.TRACK_MFMA, tier=ops.TIER_WHOLE_MAP)
    assert st["whole_map_tier"] == M, st
    _check(gc, out, gc.ref, f"whole-map tier {st}")


def test_row_table_form(gc):
    """Sources as rows of a 40-row table (src_row, emb_rows = 40 < M): corr_peaks gathers through src_row and finishes
    single-candidate sources in its own epilogue -- otherwise reached only through ModelInference.infer at 67 x 121."""
    assert gc.table.shape[0] == G.TABLE_ROWS < M and int(gc.src_row.bincount(minlength=G.TABLE_ROWS).min()) >= 7
    out, st = _run(gc, ops.TRACK_MFMA, emb=gc.table.cuda().contiguous(), src_row=gc.src_row.int().cuda())
    direct, _ = _run(gc, ops.TRACK_MFMA, emb=gc.table[gc.src_row].cuda().contiguous())
    print(f"{gc.case} table form: bits equal to the direct form: {torch.equal(out, direct)}; tiers {st}")
    err = (out - gc.ref_table).abs().max(dim=1).values
    assert torch.isfinite(out).all() and err.max() < PX_TOL, (int(err.argmax()), float(err.max()))
    print(f"{gc.case} table form: max err {float(err.max()):.2e} px")


def test_candidate_kernel_and_tier_counts(gc):
    """The kernel names of one one-round MFMA call: corr_peaks for the grids the position tag admits, corr16_peaks + select
    beyond it (and at C = 64) -- so that a change to the dispatch cannot silently move a case to the other side.  Tier counts:
    the oracle leaves nothing for the slow tiers on these inputs (CPU file), so the exact tier stays within the project's cap
    M / 20 and more than half of the sources finish on the fast tier."""
    ops.profile_enable(True)
    try:
        out, st = _run(gc, ops.TRACK_MFMA)
        names = set(ops.profile_collect())
    finally:
        ops.profile_enable(False)
    print(f"{gc.case} kernels: {sorted(names)}; tiers {st}")
    if gc.case.kernel == G.PEAKS:
        assert "corr_peaks" in names and "corr16_peaks" not in names and "select" not in names, sorted(names)
    else:
        assert "corr16_peaks" in names and "select" in names and "corr_peaks" not in names, sorted(names)
    fast = M - st["whole_map_tier"] - st["exact_tier"]
    assert st["sources"] == M and st["exact_tier"] <= M // 20, st
    assert fast > M // 2, st
    assert (out - gc.ref).abs().max() < PX_TOL   # (profiling changes nothing)


@pytest.mark.parametrize("method", [ops.TRACK_EXACT, ops.TRACK_MFMA], ids=["exact", "mfma"])
def test_argmax_cells(gc, method):
    """dtk_argmax_cells: the cell is the arg-max of the float64 cosine map for every source (top-two gap >= 3.6e-5 on these
    inputs, fp32 and float64 agree: CPU file), the cosine within 2e-6 of it."""
    trk = gc.trk[ops.TRACK_MFMA]
    feat, norms, f16 = trk.features()
    cell, cos = ops.argmax_cells(trk.geom, feat, norms, f16 if method == ops.TRACK_MFMA else None, gc.src_d, None, gc.tgt_d, method)
    torch.cuda.synchronize()
    cell, cos = cell.cpu().long(), cos.cpu().double()
    wrong = torch.nonzero(cell != gc.cos_arg)[:, 0]
    dcos = (cos - gc.cos_max).abs()
    print(f"{gc.case} argmax_cells: {wrong.numel()} cells differ, max |dcos| {float(dcos.max()):.2e}")
    assert wrong.numel() == 0, (wrong.tolist()[:10], cell[wrong][:10].tolist(), gc.cos_arg[wrong][:10].tolist())
    assert dcos.max() < COS_TOL, (int(dcos.argmax()), float(dcos.max()))


@pytest.mark.parametrize("ph,pw,form", G.EXACT_FORM_GRIDS, ids=[f"{a}x{b}" for a, b, _ in G.EXACT_FORM_GRIDS])
def test_exact_head_forms_and_grid_limit(ph, pw, form):
    """Found by the 128 x 128 and 101 x 181 cases: the exact path (TRACK_EXACT and tier 3 of TRACK_MFMA) kept map, logits and hidden
    ring of a map in LDS and refused every grid beyond 2 ph pw + 128 pw + 16 floats -- 720 x 1280 among them, and on TRACK_MFMA only
    when the first source reached tier 3.  head_exact_kernel now has a large-grid form (map read from global memory, two output
    rows per block).  Here: the last grid of the first form, the first and the last of the second -- both methods against the
    oracle, a source that must take tier 3 included -- and the first grid beyond, which both methods refuse before any work."""
    from gpu_util import make_tracker
    H, W, C, n = G.PATCH + G.STRIDE * (ph - 1), G.PATCH + G.STRIDE * (pw - 1), 32, 40
    assert A.feature_grid(H, W) == (ph, pw) and G.exact_form(ph, pw) == form
    feats = synth.synth_features(1, C, ph, pw, seed=G.FEAT_SEED)
    head = G.head_weights()
    g = torch.Generator().manual_seed(G.SRC_SEED)
    pts = torch.rand(n, 2, generator=g) * torch.tensor([W - 1.0, H - 1.0])
    tgt = torch.zeros(n, dtype=torch.long)
    src = A.sample_bilinear(feats, pts, tgt, H, W)
    src[0] = feats[0, :, ph - 1, pw - 1]   # the last cell of the map
    src[1] = 0.0                           # an all-zero map (non-positive maximum): tier 3 on the MFMA method
    for method in (ops.TRACK_EXACT, ops.TRACK_MFMA):
        trk = make_tracker(torch.zeros(1, 3, H, W), feats, head, method=method)
        out = torch.full((n, 2), float("nan"), device="cuda")
        if form == "refused":
            with pytest.raises(RuntimeError, match=f"token grid {ph}x{pw}"):
                trk.track_sources(trk.features(), src.cuda().contiguous(), None, tgt.int().cuda(), None, out, n)
            assert torch.isnan(out).all()   # refused before any source was processed
            continue
        ref = A.track(src, feats, tgt, head, H, W)
        trk.track_sources(trk.features(), src.cuda().contiguous(), None, tgt.int().cuda(), None, out, n)
        torch.cuda.synchronize()
        st = trk.last_track_stats
        err = (out.cpu() - ref).abs().max(dim=1).values
        print(f"{ph}x{pw} ({form}) method {method}: max err {float(err.max()):.2e} px, tiers {st}")
        assert method == ops.TRACK_EXACT or st["exact_tier"] >= 1, st
        assert torch.isfinite(out).all() and err.max() < PX_TOL, (method, int(err.argmax()), float(err.max()))


def test_infer_end_to_end_at_35x35():
    """ModelInference.infer at 256 x 256 (35 x 35, 93 padding cells per row), C = 384, T = 6: the row-table form plus the anchor
    bookkeeping, against A.infer."""
    from gpu_util import make_inference, make_tracker
    H = W = 256
    T, C = 6, 384
    assert A.feature_grid(H, W) == (35, 35)
    feats = synth.synth_features(T, C, 35, 35, seed=G.FEAT_SEED)
    head = G.head_weights()
    queries = synth.grid_queries(4, 3, H, W, 1)
    rt, ro, cs, _ = A.infer(feats, queries, head, H, W, return_aux=True)
    trk = make_tracker(torch.zeros(T, 3, H, W), feats, head, method=ops.TRACK_MFMA)
    ops.profile_enable(True)
    try:
        traj, occ = make_inference(trk, H, W, T).infer(queries.cuda())
        names = set(ops.profile_collect())
    finally:
        ops.profile_enable(False)
    err = (traj.cpu() - rt).abs().max()
    print(f"infer 35x35: {queries.shape[0]} queries x {T} frames, {int((cs >= 0.7).sum())} anchor pairs, max err {float(err):.2e} px, "
          f"{int((occ.cpu() != ro).sum())} flags differ, {int(ro.sum())} occluded; tiers of the anchor stage {trk.last_track_stats}")
    assert "corr_peaks" in names, sorted(names)
    assert torch.isfinite(traj).all() and err < PX_TOL
    assert torch.equal(occ.cpu(), ro)
