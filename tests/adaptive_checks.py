"""The definition of an adaptive frame, stated once for every adaptive call (a helper, not
a test): rm_dispatch_adaptive, _refine, _adaptive_edges and their pattern forms (DESIGN
§4.12, §4.15).  With A the AA-off frame, X the frame the flagged pixels take (the AA-on frame
B, or a pattern's frame P) and M the expected mask: the call's mask is M, rm_aa_refined is
M.sum(), the image is where(M, X, A) byte for byte in RGBA8 and bit for bit (as uint32) in
RGBA32F, and a G-buffer context's G-buffer is pass 1's.  A, X and G come from
tests/frames.py refs.  Also the masks, criteria and refusal checks those tests share."""
import ctypes as C

import numpy as np

from adaptive_edges_model import DEPTH, ID, NORMAL, edge_mask

E3 = ID | DEPTH | NORMAL  # rm_aa_criteria_init's
DEFAULTS = dict(color_threshold=8, depth_rel=0.05, normal_cos=0.9)


def expected(M, A, X):
    m = np.asarray(M).astype(bool)[..., None]
    return np.where(m, X[0], A[0]), np.where(m, X[1].view(np.uint32), A[1].view(np.uint32))


def check_frame(r, M_want, A, X, what, G=None):
    """The context after an adaptive dispatch, against the definition.  Returns the mask and
    the two images read (None for an output the context does not have)."""
    M = r.read_aa_mask()
    assert M.dtype == np.uint8 and M.shape == M_want.shape, \
        f"{what}: the mask is {M.dtype} {M.shape}, expected uint8 {M_want.shape}"
    np.testing.assert_array_equal(M, M_want, err_msg=f"{what}: mask")
    assert r.aa_refined() == int(M_want.sum()), f"{what}: rm_aa_refined {r.aa_refined()}, the mask flags {int(M_want.sum())}"
    w8, w32 = expected(M_want, A, X)
    c8 = c32 = None
    if r.outputs & 1:
        c8 = r.read_rgba8()
        assert c8.tobytes() == w8.tobytes(), f"{what}: rgba8, {int((c8 != w8).any(-1).sum())} pixels differ"
    if r.outputs & 2:
        c32 = r.read_rgba32f()
        np.testing.assert_array_equal(c32.view(np.uint32), w32, err_msg=f"{what}: rgba32f")
    if r.outputs & 4 and G is not None:
        assert r.read_gbuffer().tobytes() == G.tobytes(), f"{what}: the G-buffer is pass 1's"
    return M, c8, c32


# ---- masks and criteria ----------------------------------------------------------------------
def caller_masks(W, H):
    g = np.random.default_rng(20261019)
    rnd = (g.random((H, W)) < 0.5).astype(np.uint8)
    if rnd.sum() % 16 == 0:
        rnd[0, 0] ^= 1
    yy, xx = np.mgrid[0:H, 0:W]
    corners = np.zeros((H, W), np.uint8)
    corners[[0, 0, -1, -1], [0, -1, 0, -1]] = 1
    one = np.zeros((H, W), np.uint8)
    one[H // 2, W // 3] = 1
    values = rnd.copy()  # any non-zero byte flags its pixel
    values[rnd == 1] = np.where(g.random(int(rnd.sum())) < 0.5, 2, 255).astype(np.uint8)
    return {"ones": np.ones((H, W), np.uint8), "zeros": np.zeros((H, W), np.uint8),
            "checker": ((xx + yy) & 1).astype(np.uint8), "corners": corners, "one": one, "random": rnd,
            "values": values}


def some_mask(W, H, k, seed=5):
    """k flagged pixels of a W x H frame, as bytes of several non-zero values."""
    rng = np.random.default_rng(seed + k)
    m = np.zeros(W * H, np.uint8)
    m[rng.choice(W * H, k, replace=False)] = rng.choice([1, 7, 128, 255], k)
    return m.reshape(H, W)


def edges_mask(ref, W, H, edges=E3, **kw):
    """The expected mask of an edges case, never empty and never full at 9 x 5 and above."""
    with np.errstate(all="ignore"):
        M = edge_mask(ref["G"], ref["A"][0], edges, **dict(DEFAULTS, **kw))
    if (W, H) == (1, 1):
        assert not M.any(), f"1 x 1, edges {edges}: a pixel without a neighbour is flagged"
    else:
        assert 0 < int(M.sum()) < W * H, f"{W} x {H}, edges {edges}: {int(M.sum())} pixels flagged, a vacuous case"
    return M


def criteria(rm, edges, color_threshold=8, depth_rel=0.05, normal_cos=0.9, size=20):
    return rm.rm_aa_criteria(size, edges, color_threshold, depth_rel, normal_cos)


# ---- refusals ----------------------------------------------------------------------------------
ADAPTIVE_CALLS = ("rm_dispatch_adaptive", "rm_dispatch_refine", "rm_dispatch_refine_device")
PATTERN_CALLS = ("rm_dispatch_adaptive_pattern", "rm_dispatch_refine_pattern", "rm_dispatch_refine_pattern_device")


def call(rm, r, name, p, cr=None, mask=None, dev_ptr=0, pitch=0):
    """The C call itself, its status returned.  rm_dispatch_adaptive at threshold 16; the
    three older calls take no pattern and no criteria."""
    lib = rm.lib()
    host = mask.ctypes.data if mask is not None else None
    if name == "rm_dispatch_adaptive":
        return lib.rm_dispatch_adaptive(r.handle, 16)
    if name == "rm_dispatch_refine":
        return lib.rm_dispatch_refine(r.handle, host, pitch)
    if name == "rm_dispatch_refine_device":
        return lib.rm_dispatch_refine_device(r.handle, dev_ptr or None, pitch)
    pp = C.byref(p) if p is not None else None
    if name == "rm_dispatch_adaptive_pattern":
        return lib.rm_dispatch_adaptive_pattern(r.handle, C.byref(cr) if cr is not None else None, pp)
    if name == "rm_dispatch_refine_pattern":
        return lib.rm_dispatch_refine_pattern(r.handle, host, pitch, pp)
    assert name == "rm_dispatch_refine_pattern_device", f"no such call: {name}"
    return lib.rm_dispatch_refine_pattern_device(r.handle, dev_ptr or None, pitch, pp)


def refused(rm, r, code, p, cr, mask, dev_ptr, word=None, pitch=0, calls=PATTERN_CALLS):
    """Every call of `calls` returns `code`, and the context's last error starts with the
    call's own name (and holds `word`)."""
    for name in calls:
        rc = call(rm, r, name, p, cr, mask, dev_ptr, pitch)
        assert rc == code, f"{name} returned {rc}, expected {code}"
        msg = rm.lib().rm_last_error(r.handle).decode()
        assert msg.startswith(name + ": "), (name, msg)
        if word:
            assert word in msg, (name, msg)
