"""Pattern refinement in the adaptive calls on the GPU (rm_dispatch_adaptive_pattern,
rm_dispatch_refine_pattern / _device; include/rm_api.h RM_HAS_ADAPTIVE_PATTERN).

The definition.  For a frame u, a scene and a pattern p, three references come from other
calls of the same library (tests/frames.py refs): A, the AA-off rm_dispatch frame, and P, the
rm_dispatch_pattern(p) frame, both on a plain context with both colour outputs (G-buffer contexts
refuse rm_dispatch_pattern); G, the AA-off rm_dispatch G-buffer of a G-buffer context.  The expected
mask M is tests/adaptive_edges_model.py's rule on G (and A's RGBA8 under COLOR), or the mask
given.  Then the call's mask is M, rm_aa_refined is M.sum(), the frame is where(M, P, A) bit for
bit in RGBA32F and byte for byte in RGBA8, and the G-buffer is G bit for bit
(tests/adaptive_checks.py check_frame).

Frames are rm_sweep_uniforms(60, 120, ., 0, .) (tests/uniforms.py main_u).  The
shapes: 130 x 67 (several tiles, a partial last group), 37 x 23, 9 x 5, 8 x 8 and 1 x 1 (no
neighbour, nothing flagged).  Every edges case at 9 x 5 and above asserts 0 < flagged < W H on
the expected mask; tests/test_adaptive_pattern_abi.py holds the same condition against the
oracle's G-buffer on the CPU for the frames and criteria used here.
"""
import numpy as np
import pytest

from adaptive_checks import DEFAULTS, E3, call, check_frame, criteria, edges_mask, expected, refused, some_mask
from adaptive_checks import PATTERN_CALLS as CALLS
from adaptive_edges_model import COLOR, DEPTH, ID, NORMAL
from adaptive_model import flag_mask
from frames import ALL, BOTH, images, pattern_frame, refs, renderer
from patterns import equals_model, model
from patterns import refine_patterns as patterns
from scenes import scene_of
from uniforms import main_u

pytestmark = pytest.mark.gpu

SHAPES = [(130, 67), (37, 23), (9, 5), (8, 8), (1, 1)]
SCENES = ["builtin", "default-table", "random-table"]


# ---- 1. every pattern against the definition -----------------------------------------------------
SETTINGS = [(W, H, 1, 0) for W, H in SHAPES if (W, H) != (37, 23)] + [(37, 23, b, s) for b in (0, 2) for s in (0, 1)]


@pytest.mark.parametrize("W,H,bounces,shadow", SETTINGS)
def test_patterns_equal_definition(rm, gpu, W, H, bounces, shadow):
    u = main_u(rm, bounces, shadow)
    ref = refs(rm, W, H, bounces, shadow)
    M = edges_mask(ref, W, H)
    with renderer(rm, W, H, outputs=ALL) as r:
        for pname, p in patterns(rm).items():
            P = pattern_frame(rm, W, H, p, pname, bounces, shadow)
            r.dispatch_adaptive_pattern(u, None, p)
            check_frame(r, M, ref["A"], P, f"{W}x{H} b{bounces} s{shadow} {pname}", ref["G"])
        if (W, H) == (130, 67):  # the frame is neither of its two sources
            P = pattern_frame(rm, W, H, rm.sample_pattern(rm.RM_PATTERN_GRID4), "grid4", bounces, shadow)
            r.dispatch_adaptive_pattern(u, None, rm.RM_PATTERN_GRID4)
            c8 = r.read_rgba8()
            assert (c8 != ref["A"][0]).any() and (c8 != P[0]).any()
        # u.AA is ignored, and the uniforms stay as they are
        u_on = main_u(rm, bounces, shadow, True)
        r.dispatch_adaptive_pattern(u_on, None, rm.RM_PATTERN_GRID3)
        assert bytes(r.get_uniforms()) == bytes(u_on)
        check_frame(r, M, ref["A"], pattern_frame(rm, W, H, rm.sample_pattern(rm.RM_PATTERN_GRID3), "grid3", bounces, shadow),
                    "u.AA = 1", ref["G"])


# ---- 2. against the rule directly: a fault shared with k_pattern cannot hide -----------------------
@pytest.mark.parametrize("pname", ["grid3", "abs7"])
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_flagged_pixels_equal_the_rule(rm, oracle, gpu, name, pname):
    """The flagged pixels against tests/sample_pattern_model.py over SHADE traces of the same
    context (tests/patterns.py model), the others against A."""
    W, H = 37, 23
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0, name)
    M = edges_mask(ref, W, H).astype(bool)
    p = patterns(rm)[pname]
    with renderer(rm, W, H, scene_of(rm, name), outputs=ALL) as r:
        r.dispatch_adaptive_pattern(u, None, p)
        g8, g32 = images(r)
        np.testing.assert_array_equal(r.read_aa_mask().astype(bool), M)
        m8, m32 = model(rm, oracle, r, u, p)
    equals_model((g8[M], g32[M]), (m8[M], m32[M]), f"{name} {pname}: flagged")
    assert (g32[M][..., 3] == 1.0).all()
    assert g8[~M].tobytes() == ref["A"][0][~M].tobytes() and g32[~M].tobytes() == ref["A"][1][~M].tobytes()


# ---- 3. anchors ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("W,H", [(130, 67), (37, 23), (9, 5)])
def test_reference_pattern_is_adaptive_edges(rm, gpu, W, H):
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0)
    p = rm.sample_pattern(rm.RM_PATTERN_REFERENCE)
    with renderer(rm, W, H, outputs=ALL) as e, renderer(rm, W, H, outputs=ALL) as r:
        # (at 9 x 5 COLOR flags every pixel of this frame: the geometric criteria alone there)
        for edges in (E3, COLOR, E3 | COLOR) if W > 9 else (E3, ID, DEPTH):
            edges_mask(ref, W, H, edges)
            e.dispatch_adaptive_edges(u, edges, **DEFAULTS)
            r.dispatch_adaptive_pattern(u, dict(DEFAULTS, edges=edges), p)
            np.testing.assert_array_equal(r.read_aa_mask(), e.read_aa_mask())
            assert r.aa_refined() == e.aa_refined()
            assert r.read_rgba8().tobytes() == e.read_rgba8().tobytes(), edges
            assert r.read_rgba32f().tobytes() == e.read_rgba32f().tobytes(), edges
            assert r.read_gbuffer().tobytes() == e.read_gbuffer().tobytes(), edges


def test_reference_pattern_is_dispatch_refine(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 2)
    p = rm.sample_pattern(rm.RM_PATTERN_REFERENCE)
    with renderer(rm, W, H) as e, renderer(rm, W, H) as r:
        for k in (1, 100, W * H):
            m = some_mask(W, H, k)
            e.dispatch_refine(m, u)
            r.dispatch_refine_pattern(m, p, u)
            np.testing.assert_array_equal(r.read_aa_mask(), (m != 0).astype(np.uint8))
            np.testing.assert_array_equal(r.read_aa_mask(), e.read_aa_mask())
            assert r.read_rgba8().tobytes() == e.read_rgba8().tobytes(), k
            assert r.read_rgba32f().tobytes() == e.read_rgba32f().tobytes(), k


@pytest.mark.parametrize("W,H", [(130, 67), (37, 23), (1, 1)])
def test_all_ones_mask_is_the_pattern_frame(rm, gpu, W, H):
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0)
    ones = np.full((H, W), 255, np.uint8)
    with renderer(rm, W, H) as r:
        for pname, p in patterns(rm).items():
            P = pattern_frame(rm, W, H, p, pname, 2, 0)
            r.dispatch_refine_pattern(ones, p, u)
            assert r.aa_refined() == W * H
            assert r.read_rgba8().tobytes() == P[0].tobytes(), pname
            assert r.read_rgba32f().tobytes() == P[1].tobytes(), pname
            check_frame(r, np.ones((H, W), np.uint8), ref["A"], P, f"{W}x{H} ones {pname}", ref["G"])


def test_nothing_flagged_is_the_plain_frame(rm, gpu):
    """An all-zero mask, COLOR at threshold 255, and one sample at (0, 0) whatever is flagged."""
    W, H = 37, 23
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0)
    g4 = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    zero = np.zeros((H, W), np.uint8)
    with renderer(rm, W, H) as r:
        for p in (g4, patterns(rm)["jitter1"]):
            r.dispatch_refine_pattern(zero, p, u)
            check_frame(r, zero, ref["A"], ref["A"], "zero mask", ref["G"])
            r.dispatch_adaptive_pattern(u, dict(edges=COLOR, color_threshold=255), p)
            check_frame(r, zero, ref["A"], ref["A"], "threshold 255", ref["G"])
    centre = patterns(rm)["centre"]
    with renderer(rm, W, H, outputs=ALL) as r:
        M = edges_mask(ref, W, H)
        r.dispatch_adaptive_pattern(u, None, centre)
        check_frame(r, M, ref["A"], ref["A"], "centre, edges", ref["G"])
        ones = np.ones((H, W), np.uint8)
        r.dispatch_refine_pattern(ones, centre)
        check_frame(r, ones, ref["A"], ref["A"], "centre, all ones", ref["G"])


@pytest.mark.parametrize("pname", ["jitter1", "grid3"])
def test_group_ends(rm, gpu, pname):
    """Lists of 1, 15, 16, 17, 63, 64 and 65 entries: the ends of the groups of 16 (n > 1) and of
    64 (n = 1), a full group and one entry more."""
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    p = patterns(rm)[pname]
    P = pattern_frame(rm, W, H, p, pname, 1, 0)
    with renderer(rm, W, H) as r:
        for k in (1, 15, 16, 17, 63, 64, 65):
            m = some_mask(W, H, k)
            r.dispatch_refine_pattern(m, p, u)
            check_frame(r, (m != 0).astype(np.uint8), ref["A"], P, f"{pname} {k} flagged", ref["G"])


# ---- 4. one wave strides over every group: the LDS sum is reused between groups -------------------
@pytest.mark.parametrize("pname", ["grid3", "jitter1"])
def test_one_wave_walks_every_group(rm, gpu, monkeypatch, pname):
    W, H = 37, 23  # 851 pixels: 54 groups of 16, 14 groups of 64
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    p = patterns(rm)[pname]
    P = pattern_frame(rm, W, H, p, pname, 1, 0)
    monkeypatch.setenv("RM_AA_REFINE_WAVES", "1")
    with renderer(rm, W, H) as r:
        monkeypatch.delenv("RM_AA_REFINE_WAVES")  # read at rm_create
        ones = np.ones((H, W), np.uint8)
        r.dispatch_refine_pattern(ones, p, u)
        check_frame(r, ones, ref["A"], P, f"one wave, {pname}", ref["G"])
        m = some_mask(W, H, 333)
        r.dispatch_refine_pattern(m, p)
        check_frame(r, (m != 0).astype(np.uint8), ref["A"], P, f"one wave, {pname}, 333 flagged", ref["G"])


# ---- 5. the sum follows the pattern's order ------------------------------------------------------------
def test_sample_order_is_the_sum_order(rm, oracle, gpu):
    W, H = 37, 23
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0)
    M = edges_mask(ref, W, H).astype(bool)
    g4 = rm.sample_pattern(rm.RM_PATTERN_GRID4)
    perm = np.random.default_rng(4).permutation(16)
    pp = rm.custom_pattern([g4.dx[i] for i in perm], [g4.dy[i] for i in perm])
    with renderer(rm, W, H, outputs=ALL) as r:
        r.dispatch_adaptive_pattern(u, None, g4)
        f1 = images(r)
        m1 = model(rm, oracle, r, u, g4)
        r.dispatch_adaptive_pattern(u, None, pp)
        f2 = images(r)
        m2 = model(rm, oracle, r, u, pp)
    equals_model((f1[0][M], f1[1][M]), (m1[0][M], m1[1][M]), "grid4")
    equals_model((f2[0][M], f2[1][M]), (m2[0][M], m2[1][M]), "grid4 permuted")
    ok = ~(np.isnan(m1[1]) | np.isnan(m2[1])) & M[..., None]
    dm = m1[1].view(np.uint32) ^ m2[1].view(np.uint32)
    assert dm[ok].any(), "the two orders round differently somewhere on the flagged pixels"
    df = f1[1].view(np.uint32) ^ f2[1].view(np.uint32)
    np.testing.assert_array_equal(df[ok], dm[ok])
    assert not df[~M].any(), "the pixels that are not flagged are pass 1's in both"


# ---- 6. scene tables, generic and specialised --------------------------------------------------------------
@pytest.mark.parametrize("specialize", [False, True], ids=["generic", "specialised"])
@pytest.mark.parametrize("name", ["default-table", "random-table"])
def test_tables(rm, gpu, name, specialize):
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0, name)
    M = edges_mask(ref, W, H)
    with renderer(rm, W, H, scene_of(rm, name), outputs=ALL, specialize=specialize) as r:
        for pname in ("grid3", "grid4", "reference", "jitter1"):
            p = patterns(rm)[pname]
            r.dispatch_adaptive_pattern(u, None, p)
            check_frame(r, M, ref["A"], pattern_frame(rm, W, H, p, pname, 1, 0, name), f"{name} {pname}", ref["G"])
        ones = np.ones((H, W), np.uint8)
        for pname in ("abs7", "jitter1"):
            p = patterns(rm)[pname]
            r.dispatch_refine_pattern(ones, p)
            check_frame(r, ones, ref["A"], pattern_frame(rm, W, H, p, pname, 1, 0, name), f"{name} ones {pname}", ref["G"])
    if name == "default-table":  # the default table is the built-in scene
        assert refs(rm, W, H, 1, 0)["G"].tobytes() == ref["G"].tobytes()


# ---- 7. contexts ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("outputs", [1, 2, 3, 1 | 4, 2 | 4, 3 | 4],
                         ids=["rgba8", "rgba32f", "both", "rgba8+g", "rgba32f+g", "both+g"])
def test_outputs(rm, gpu, outputs):
    """COLOR reads the RGBA8 image or quantises the RGBA32F one; the geometric criteria need the
    G-buffer.  Both refine kernels (GRID3, one jittered sample)."""
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    with renderer(rm, W, H, outputs=outputs) as r:
        for edges in (COLOR,) + ((E3, E3 | COLOR) if outputs & 4 else ()):
            M = edges_mask(ref, W, H, edges)
            for pname in ("grid3", "jitter1"):
                p = patterns(rm)[pname]
                r.dispatch_adaptive_pattern(u, dict(DEFAULTS, edges=edges), p)
                check_frame(r, M, ref["A"], pattern_frame(rm, W, H, p, pname, 1, 0), f"outputs {outputs} edges {edges} {pname}", ref["G"])
    if outputs == 3:  # COLOR alone is rm_dispatch_adaptive's rule
        np.testing.assert_array_equal(M, flag_mask(ref["A"][0], 8))


def test_mask_calls_on_a_gbuffer_context(rm, gpu):
    """A host mask with a pitch, and a device mask that is the context's own copy."""
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    pats = patterns(rm)
    wide = np.zeros((H, W + 5), np.uint8)
    wide[:, W:] = 9  # the padding is not read as pixels
    wide[:, :W] = some_mask(W, H, 200)
    m = wide[:, :W]
    want = (m != 0).astype(np.uint8)
    with renderer(rm, W, H, outputs=ALL) as r:
        r.dispatch_refine_pattern(m, pats["grid4"], u)  # row_pitch W + 5
        check_frame(r, want, ref["A"], pattern_frame(rm, W, H, pats["grid4"], "grid4", 1, 0), "host mask", ref["G"])
        ptr = r.aa_mask_ptr()
        for pname in ("grid3", "jitter1"):
            r.dispatch_refine_pattern(ptr, pats[pname], None, 0)  # its own normalised copy
            check_frame(r, want, ref["A"], pattern_frame(rm, W, H, pats[pname], pname, 1, 0), f"own mask {pname}", ref["G"])
        assert r.aa_mask_ptr() == ptr
        # a G-buffer criterion of the caller's own: the floor's pixels, from the records just written
        own = (r.read_gbuffer()["id"] == 7).astype(np.uint8)
        assert 0 < own.sum() < W * H
        r.dispatch_refine_pattern(own, pats["grid3"])
        check_frame(r, own, ref["A"], pattern_frame(rm, W, H, pats["grid3"], "grid3", 1, 0), "own criterion", ref["G"])


def test_caller_owned_images_and_stream(rm, gpu):
    import torch
    W, H = 37, 23
    u, u2 = main_u(rm, 1), rm.sweep_uniforms(20, 120, 1, False, 0)
    ref = refs(rm, W, H, 1, 0)
    M = edges_mask(ref, W, H)
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    P = pattern_frame(rm, W, H, p, "grid3", 1, 0)
    with renderer(rm, W, H, outputs=ALL) as r:
        dev = torch.device("cuda", r.device)
        s = torch.cuda.Stream(device=dev)
        r.dispatch(u2)  # the context's own images hold another frame
        stale_g, stale8 = r.read_gbuffer(), r.read_rgba8()
        try:
            with torch.cuda.stream(s):
                r.set_stream(s.cuda_stream)
                buf = torch.full((H * W * 8 + 8,), -7.25, dtype=torch.float32, device=dev)
                out = torch.zeros((H, W, 4), dtype=torch.uint8, device=dev)
                r.set_output_gbuffer(buf.data_ptr())
                r.set_output_rgba8(out.data_ptr())
                r.dispatch_adaptive_pattern(u, None, p)  # the table's upload is on s too
                got8, gotg = out.cpu().numpy(), buf.cpu().numpy()  # ordered after the frame on the stream
            r.synchronize()
            assert gotg[:H * W * 8].tobytes() == ref["G"].tobytes(), "the caller's buffer holds pass 1's records"
            assert (gotg[H * W * 8:] == np.float32(-7.25)).all(), "the sentinel after the last record"
            assert got8.tobytes() == expected(M, ref["A"], P)[0].tobytes()
            check_frame(r, M, ref["A"], P, "caller-owned", ref["G"])
        finally:
            r.synchronize()
            r.set_output_gbuffer(None)
            r.set_output_rgba8(None)
            r.set_stream(None)
        assert r.read_gbuffer().tobytes() == stale_g.tobytes(), "the context's own G-buffer was left alone"
        assert r.read_rgba8().tobytes() == stale8.tobytes(), "and its own image"


# ---- 8. nothing sticky --------------------------------------------------------------------------------------------
def test_nothing_sticky(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 1)
    u_on = main_u(rm, 1, 0, True)
    ref = refs(rm, W, H, 1, 0)
    M = edges_mask(ref, W, H)
    pats = patterns(rm)
    with renderer(rm, W, H, outputs=ALL) as fresh:
        fresh.dispatch(u_on)
        want_on = images(fresh) + (fresh.read_gbuffer(),)
        fresh.dispatch_adaptive_edges(u, E3)
        want_edges = images(fresh)
    with renderer(rm, W, H, outputs=ALL) as r:
        r.dispatch_adaptive_pattern(u_on, None, pats["grid4"])
        check_frame(r, M, ref["A"], pattern_frame(rm, W, H, pats["grid4"], "grid4", 1, 0), "first", ref["G"])
        assert bytes(r.get_uniforms()) == bytes(u_on)
        r.dispatch()  # the plain AA-on frame, as always, with the first sample's G-buffer
        assert images(r)[0].tobytes() == want_on[0].tobytes() and images(r)[1].tobytes() == want_on[1].tobytes()
        assert r.read_gbuffer().tobytes() == want_on[2].tobytes()
        np.testing.assert_array_equal(r.read_aa_mask(), M)  # the mask stays the last adaptive dispatch's
        r.dispatch_adaptive_edges(u, E3)
        assert images(r)[0].tobytes() == want_edges[0].tobytes() and images(r)[1].tobytes() == want_edges[1].tobytes()
        for pname in ("grid3", "jitter1", "grid4", "grid4", "abs7", "grid3"):  # patterns in turn
            r.dispatch_adaptive_pattern(None, None, pats[pname])
            check_frame(r, M, ref["A"], pattern_frame(rm, W, H, pats[pname], pname, 1, 0), f"in turn: {pname}", ref["G"])
        r.dispatch(u)
        assert r.read_rgba8().tobytes() == ref["A"][0].tobytes() and r.read_gbuffer().tobytes() == ref["G"].tobytes()
    # a plain context: rm_dispatch_pattern afterwards, and the table's cache shared by both kinds of call
    g2, g4 = pats["grid2"], pats["grid4"]
    P2, P4 = pattern_frame(rm, W, H, g2, "grid2", 1, 0), pattern_frame(rm, W, H, g4, "grid4", 1, 0)
    m = some_mask(W, H, 300)
    with renderer(rm, W, H) as r:
        for i in range(3):
            r.dispatch_pattern(u, g2)
            assert r.read_rgba8().tobytes() == P2[0].tobytes() and r.read_rgba32f().tobytes() == P2[1].tobytes(), i
            r.dispatch_refine_pattern(m, g4)
            check_frame(r, (m != 0).astype(np.uint8), ref["A"], P4, f"alternating {i}", ref["G"])
        r.dispatch_pattern(None, g4)  # the refinement's table, not uploaded again: the same frame
        assert r.read_rgba8().tobytes() == P4[0].tobytes() and r.read_rgba32f().tobytes() == P4[1].tobytes()
        r.dispatch_refine_pattern(m, g4)
        check_frame(r, (m != 0).astype(np.uint8), ref["A"], P4, "after rm_dispatch_pattern of the same pattern", ref["G"])


# ---- 9. offsets far outside the pixel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["builtin", "random-table"])
def test_sixteen_pixel_offsets(rm, oracle, gpu, name):
    """+-16 pixels: the refinement's |rd| = 1 proof (Frame::unit_rd) is taken over the pattern's uv
    range, not pass 1's.  No camera was found for which rm::unit_rd_check differs between the two
    ranges: it holds over both for all 120 sweep frames and all 256 cases of
    tests/test_gpu_fuzz_uniforms.py, at 37 x 23 and at 67 x 41.  The case stays: the frame against
    the definition, and the flagged pixels against the rule over SHADE traces."""
    W, H = 37, 23
    u = main_u(rm, 2)
    ref = refs(rm, W, H, 2, 0, name)
    M = edges_mask(ref, W, H)
    p = rm.custom_pattern([16.0, -16.0, 16.0, -16.0], [16.0, 16.0, -16.0, -16.0])
    with renderer(rm, W, H, scene_of(rm, name), outputs=ALL) as r:
        r.dispatch_adaptive_pattern(u, None, p)
        check_frame(r, M, ref["A"], pattern_frame(rm, W, H, p, "pm16", 2, 0, name), f"{name} +-16", ref["G"])
        got = images(r)
        m8, m32 = model(rm, oracle, r, u, p)
    b = M.astype(bool)
    equals_model((got[0][b], got[1][b]), (m8[b], m32[b]), f"{name} +-16: flagged")
    assert got[0][b].tobytes() != ref["A"][0][b].tobytes()


# ---- 10. timing -------------------------------------------------------------------------------------------------------
def test_one_timed_launch_per_call(rm, gpu):
    W, H = 37, 23
    u = main_u(rm, 1)
    with renderer(rm, W, H, outputs=ALL) as r:
        r.enable_timing(True)
        _, n0 = r.kernel_time_ms()
        r.dispatch_adaptive_pattern(u, None, rm.RM_PATTERN_GRID4)  # a new table: uploaded before the pair
        ms, n1 = r.kernel_time_ms()
        assert n1 - n0 == 1 and ms > 0.0
        r.dispatch_adaptive_pattern(None, None, rm.RM_PATTERN_GRID3)
        r.dispatch_adaptive_pattern(None, None, rm.RM_PATTERN_GRID3)
        r.dispatch_refine_pattern(np.ones((H, W), np.uint8), patterns(rm)["jitter1"])
        r.dispatch_refine_pattern(r.aa_mask_ptr(), rm.RM_PATTERN_GRID2)
        _, n2 = r.kernel_time_ms()
        assert n2 - n1 == 4
        assert r.frame_phases()["render_ms"] > 0.0


# ---- 11. refusals -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["counters", "nshards", "graph", "ngpus", "gbuffer_only", "no_gbuffer"])
def test_refused_contexts(rm, gpu, kind):
    import torch
    W, H = 64, 48
    u = main_u(rm)
    kw = {"counters": dict(outputs=BOTH, counters=True), "nshards": dict(outputs=BOTH, nshards=2, shard=0, row_block=8),
          "graph": dict(outputs=BOTH), "ngpus": dict(outputs=1, ngpus=1, row_block=8),
          "gbuffer_only": dict(outputs=rm.RM_OUT_GBUFFER), "no_gbuffer": dict(outputs=BOTH)}[kind]
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    mask = np.ones((H, W), np.uint8)
    with rm.Renderer(W, H, outputs=BOTH) as plain:
        plain.dispatch(u)
        want = plain.read_rgba8()
    with rm.Renderer(W, H, **kw) as r:
        dev = torch.ones((H, W), dtype=torch.uint8, device=f"cuda:{max(r.device, 0)}")
        torch.cuda.synchronize()
        if kind == "graph":
            r.graph_enable(True)
        r.set_uniforms(u)
        if kind == "no_gbuffer":  # the geometric criteria alone: the mask calls and COLOR work
            for e in (ID, DEPTH, NORMAL, rm.RM_AA_EDGE_ALBEDO, COLOR | ID):
                refused(rm, r, rm.RM_ERR_STATE, p, criteria(rm, e), mask, dev.data_ptr(), "RM_OUT_GBUFFER", calls=CALLS[:1])
        else:
            cr = criteria(rm, COLOR if kind != "gbuffer_only" else ID)
            refused(rm, r, rm.RM_ERR_STATE, p, cr, mask, dev.data_ptr())
        # the context renders correctly afterwards
        r.dispatch(u)
        if kind == "gbuffer_only":
            assert (r.read_gbuffer()["t"] != np.float32(-1.0)).any()
        elif kind in ("nshards", "ngpus"):
            assert r.read_rgba8().any()
        else:
            assert r.read_rgba8().tobytes() == want.tobytes()
        if kind in ("graph", "no_gbuffer"):  # with the graph off again, or with COLOR alone, the calls work
            if kind == "graph":
                r.graph_enable(False)
            r.dispatch_adaptive_pattern(u, dict(edges=COLOR, color_threshold=255), p)
            assert r.read_rgba8().tobytes() == want.tobytes() and r.aa_refined() == 0
            r.dispatch_refine_pattern(np.zeros((H, W), np.uint8), p)
            assert r.read_rgba8().tobytes() == want.tobytes() and r.aa_refined() == 0


def test_refused_patterns(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    M = edges_mask(ref, W, H)
    ok = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    P = pattern_frame(rm, W, H, ok, "grid3", 1, 0)
    mask = np.ones((H, W), np.uint8)
    with renderer(rm, W, H, outputs=ALL) as r:
        dev = torch.ones((H, W), dtype=torch.uint8, device=f"cuda:{max(r.device, 0)}")
        torch.cuda.synchronize()
        cr = criteria(rm, E3)
        r.dispatch_adaptive_pattern(u, cr, ok)
        args = (cr, mask, dev.data_ptr())
        refused(rm, r, rm.RM_ERR_INVALID, None, *args, "pattern")
        for field, bad, word in (("struct_size", 136, "struct_size"), ("flags", 2, "flags"), ("n", 0, "n must"),
                                 ("n", 17, "n must")):
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            setattr(p, field, bad)
            refused(rm, r, rm.RM_ERR_INVALID, p, *args, word)
        for v in (float("nan"), float("inf"), 16.5, -17.0):
            for at in (0, 8):
                p = rm.rm_sample_pattern.from_buffer_copy(ok)
                p.dy[at] = v
                refused(rm, r, rm.RM_ERR_INVALID, p, *args, "offset")
            p = rm.rm_sample_pattern.from_buffer_copy(ok)
            p.dx[9] = v  # at index n: not read
            for name in CALLS:
                assert call(rm, r, name, p, *args) == rm.RM_OK, (name, v)
            r.dispatch_adaptive_pattern(None, cr, p)
            check_frame(r, M, ref["A"], P, f"a bad offset at index n ({v})", ref["G"])
        # the context's last frame is untouched by a refusal
        before = images(r)
        refused(rm, r, rm.RM_ERR_INVALID, None, *args)
        assert images(r)[0].tobytes() == before[0].tobytes() and images(r)[1].tobytes() == before[1].tobytes()


def test_refused_criteria_and_masks(rm, gpu):
    import torch
    W, H = 37, 23
    u = main_u(rm, 1)
    ref = refs(rm, W, H, 1, 0)
    M = edges_mask(ref, W, H)
    p = rm.sample_pattern(rm.RM_PATTERN_GRID3)
    P = pattern_frame(rm, W, H, p, "grid3", 1, 0)
    nan = float("nan")
    bad = [("null criteria", None, "null criteria"), ("edges = 0", criteria(rm, 0), "edges"),
           ("an unknown bit", criteria(rm, ID | 32), "edges"), ("struct_size + 4", criteria(rm, ID, size=24), "struct_size"),
           ("color_threshold 256", criteria(rm, COLOR, color_threshold=256), "color_threshold"),
           ("depth_rel -1", criteria(rm, DEPTH, depth_rel=-1.0), "depth_rel"),
           ("depth_rel NaN", criteria(rm, DEPTH | ID, depth_rel=nan), "depth_rel"),
           ("normal_cos 2", criteria(rm, NORMAL, normal_cos=2.0), "normal_cos")]
    mask = np.ones((H, W), np.uint8)
    with renderer(rm, W, H, outputs=ALL) as r:
        dev = torch.ones((H, W), dtype=torch.uint8, device=f"cuda:{max(r.device, 0)}")
        torch.cuda.synchronize()
        r.set_uniforms(u)
        for what, cr, word in bad:
            refused(rm, r, rm.RM_ERR_INVALID, p, cr, mask, dev.data_ptr(), word, calls=CALLS[:1])
        # a bad value is not read when its bit is clear
        r.dispatch_adaptive_pattern(None, criteria(rm, E3, color_threshold=256), p)
        check_frame(r, M, ref["A"], P, "color_threshold 256 with COLOR clear", ref["G"])
        # masks: null, and a pitch below a row
        refused(rm, r, rm.RM_ERR_INVALID, p, None, None, 0, "null mask", calls=CALLS[1:])
        refused(rm, r, rm.RM_ERR_INVALID, p, None, mask, dev.data_ptr(), "row_pitch", pitch=W - 1, calls=CALLS[1:])
        check_frame(r, M, ref["A"], P, "after the refusals", ref["G"])
