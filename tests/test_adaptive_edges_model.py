"""The numpy model of rm_dispatch_adaptive_edges' flagging rule (tests/adaptive_edges_model.py)
pinned two ways: on hand-made records, where every clause of the rule of include/rm_api.h
decides a case, and on the CPU oracle's G-buffer of rm_sweep_uniforms(60, 120, 1, 0, 0),
whose flagged counts under the rule as written are the table below.  The GPU tests compare
the kernel's mask with the same model.  No GPU needed."""
import numpy as np
import pytest

from adaptive_edges_model import ALBEDO, BITS, COLOR, COUNTS, DEPTH, ID, NORMAL, edge_mask
from records import oracle_gbuffer
from uniforms import main_u

F32 = np.float32
GEOMETRY = ID | DEPTH | NORMAL | ALBEDO
MISSES_130x67 = 3565  # tests/test_gpu_gbuffer.py MISSES[False]

def records(rm, rows):
    """A (1, len(rows)) G-buffer of (t, id, normal, albedo) tuples."""
    g = np.zeros((1, len(rows)), rm.GBUFFER_DTYPE)
    for i, (t, idx, n, a) in enumerate(rows):
        g[0, i] = (t, idx, n, a)
    return g


UP, WHITE = (0.0, 1.0, 0.0), (1.0, 1.0, 1.0)


# ---- hand-made records -------------------------------------------------------------------------
def test_equality_at_each_threshold_does_not_flag(rm):
    # depth: |4 - 5| = 1 = 0.25 * min(4, 5), exactly, in float32
    g = records(rm, [(4.0, 1, UP, WHITE), (5.0, 1, UP, WHITE)])
    assert edge_mask(g, None, DEPTH, depth_rel=0.25).sum() == 0
    assert edge_mask(g, None, DEPTH, depth_rel=float(np.nextafter(F32(0.25), F32(0)))).sum() == 2
    # normal: dot = (0 * 0 + 1 * 0.5) + 0 * 0 = 0.5, exactly
    g = records(rm, [(4.0, 1, UP, WHITE), (4.0, 1, (0.0, 0.5, 0.0), WHITE)])
    assert edge_mask(g, None, NORMAL, normal_cos=0.5).sum() == 0
    assert edge_mask(g, None, NORMAL, normal_cos=float(np.nextafter(F32(0.5), F32(1)))).sum() == 2
    # colour: a difference of exactly the threshold (rm_dispatch_adaptive's rule)
    img = np.zeros((1, 2, 4), np.uint8)
    img[0, 1, 0] = 8
    assert edge_mask(None, img, COLOR, color_threshold=8).sum() == 0
    assert edge_mask(None, img, COLOR, color_threshold=7).sum() == 2
    # equal ids, equal albedos
    assert edge_mask(g, None, ID | ALBEDO).sum() == 0


def test_each_criterion_reads_its_own_field(rm):
    base = (4.0, 1, UP, WHITE)
    other = {ID: (4.0, 2, UP, WHITE), DEPTH: (8.0, 1, UP, WHITE), NORMAL: (4.0, 1, (1.0, 0.0, 0.0), WHITE),
             ALBEDO: (4.0, 1, UP, (1.0, 1.0, 0.5))}
    for bit, rec in other.items():
        g = records(rm, [base, rec, rec])
        for sel in (ID, DEPTH, NORMAL, ALBEDO):
            want = [1, 1, 0] if sel == bit else [0, 0, 0]
            assert edge_mask(g, None, sel).tolist() == [want], (bit, sel)
        assert edge_mask(g, None, GEOMETRY).tolist() == [[1, 1, 0]]


def test_a_nan_normal_does_not_flag_under_normal(rm):
    nan = float("nan")
    g = records(rm, [(4.0, 1, UP, WHITE), (4.0, 1, (nan, nan, nan), WHITE), (4.0, 1, (1.0, 0.0, 0.0), WHITE)])
    assert edge_mask(g, None, NORMAL).sum() == 0  # NaN < normal_cos is false, on both of its pairs
    # a NaN albedo passes !=, a NaN depth is a hit whose difference fails >
    g = records(rm, [(4.0, 1, UP, WHITE), (nan, 1, UP, (nan, 1.0, 1.0))])
    assert edge_mask(g, None, ALBEDO).sum() == 2
    assert edge_mask(g, None, DEPTH, depth_rel=0.0).sum() == 0


def test_a_hit_beside_a_miss_flags_under_id_only(rm):
    miss = (-1.0, -1, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0))
    g = records(rm, [(4.0, 1, UP, (0.0, 0.0, 0.0)), miss, miss])
    assert edge_mask(g, None, ID).tolist() == [[1, 1, 0]]
    # "both hit" fails: no depth and no normal edge, though |4 - -1| and the dot 0 would pass
    assert edge_mask(g, None, DEPTH, depth_rel=0.0).sum() == 0
    assert edge_mask(g, None, NORMAL, normal_cos=1.0).sum() == 0
    assert edge_mask(g, None, ALBEDO).sum() == 0  # (this hit's albedo is the miss's)


@pytest.mark.parametrize("W,H", sorted(COUNTS))
def test_the_mask_is_symmetric(rm, oracle, W, H):
    """If q flags p, p flags q: a flagged pixel has a flagged 4-neighbour."""
    g = oracle_gbuffer(rm, oracle, main_u(rm), W, H)
    for edges in list(BITS.values()) + [GEOMETRY]:
        m = edge_mask(g, None, edges).astype(bool)
        n = np.zeros_like(m)
        n[:, 1:] |= m[:, :-1]
        n[:, :-1] |= m[:, 1:]
        n[1:] |= m[:-1]
        n[:-1] |= m[1:]
        assert m.any() and n[m].all(), edges
        # and the rule does not care which way the frame is scanned
        assert (edge_mask(g[::-1, ::-1], None, edges)[::-1, ::-1] == m).all(), edges


def test_one_pixel_has_no_neighbour(rm, oracle):
    g = oracle_gbuffer(rm, oracle, main_u(rm), 130, 67)[33:34, 60:61]
    img = np.full((1, 1, 4), 200, np.uint8)
    for edges in (COLOR, ID, DEPTH, NORMAL, ALBEDO, GEOMETRY | COLOR):
        assert edge_mask(g, img, edges, 0, 0.0, 1.0).sum() == 0


@pytest.mark.parametrize("W,H", sorted(COUNTS))
def test_infinite_depth_rel_flags_nothing(rm, oracle, W, H):
    g = oracle_gbuffer(rm, oracle, main_u(rm), W, H)
    assert edge_mask(g, None, DEPTH, depth_rel=float("inf")).sum() == 0
    assert edge_mask(g, None, DEPTH, depth_rel=0.0).sum() >= COUNTS[(W, H)]["DEPTH"]  # (a wider net)


# ---- the oracle's G-buffer ---------------------------------------------------------------------
@pytest.mark.parametrize("W,H", sorted(COUNTS))
def test_counts_on_the_oracle_gbuffer(rm, oracle, W, H):
    g = oracle_gbuffer(rm, oracle, main_u(rm), W, H)
    assert not np.isnan(g["normal"]).any()
    got = {k: int(edge_mask(g, None, b, depth_rel=0.05, normal_cos=0.9).sum()) for k, b in BITS.items()}
    print(f"{W}x{H}: {got}")
    assert got == COUNTS[(W, H)]
    for k, n in got.items():  # every criterion alone: a non-empty proper subset
        assert 0 < n < W * H, k
    if (W, H) == (130, 67):
        assert int((g["t"] == F32(-1.0)).sum()) == MISSES_130x67
        share = edge_mask(g, None, GEOMETRY, depth_rel=0.05, normal_cos=0.9).mean()
        assert round(float(share), 4) == 0.4385, share


def test_union_is_the_union(rm, oracle):
    g = oracle_gbuffer(rm, oracle, main_u(rm), 37, 23)
    each = [edge_mask(g, None, b) for b in BITS.values()]
    assert (edge_mask(g, None, GEOMETRY) == np.bitwise_or.reduce(each)).all()
    img = np.zeros((23, 37, 4), np.uint8)
    img[5, 7, 2] = 90
    assert (edge_mask(g, img, ID | COLOR) == (each[0] | edge_mask(None, img, COLOR))).all()
