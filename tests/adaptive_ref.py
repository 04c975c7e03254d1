"""A plain numpy restatement of adaptive supersampling (rt_set_adaptive, include/rt_api.h).

B is the dispatch's one-sample frame and S its n x n frame (ss_ref.box of the sample frame),
both over the dispatch's own pixels: compact rows r whose image row y_of_row[r] lies inside
the frame. Pixels (r, x) and (r, x + 1) are neighbours; (r, x) and (r + 1, x) are neighbours
iff y_of_row[r + 1] == y_of_row[r] + 1 (no neighbour across the gap between two stripes).
A pixel is refined iff !(|B(p).c - B(q).c| <= threshold), one float32 subtraction, for some
neighbour q and some channel c of R, G, B; the frame is S where refined and B elsewhere.
"""
import numpy as np

# the oracle cases of tests/test_adaptive_cpu.py and tests/test_gpu_adaptive.py:
# cfg, W, H, n, (maxBounces, useBVH, useFresnel, useMollerTrumbore)
ORACLE_CASES = [
    (1, 80, 60, 2, (3, True, False, False)),
    (1, 40, 30, 4, (3, True, False, False)),
    (1, 20, 15, 8, (3, True, False, False)),
    (2, 100, 75, 2, (1, True, False, False)),
    (2, 100, 75, 2, (4, True, True, False)),
    (3, 96, 54, 2, (3, True, False, False)),
    (3, 64, 40, 4, (3, True, False, False)),
]
THRESHOLD = np.float32(1.0 / 16.0)
NEAR = 2e-4        # two pixels each within the parity tolerance 1e-4 move a contrast by 2e-4
NEAR_CAP = 0.002   # at most 0.2 % of the pixels may lie that near the threshold


def rows_of(height, y0, stripe, period, out_rows):
    """Image row of every compact row of rt_dispatch_rows_ex (rows at or past `height` included)."""
    r = np.arange(out_rows, dtype=np.int64)
    return y0 + (r // stripe) * period + r % stripe


def contrast(B, y_of_row):
    """float32 (rows, width): per pixel the largest |B(p).c - B(q).c| over its neighbours q and the
    channels R, G, B, each one float32 subtraction; NaN where any of them is NaN (np.maximum
    keeps it), 0 for a pixel without neighbours."""
    B = np.asarray(B, np.float32)[..., :3]
    y = np.asarray(y_of_row, np.int64)
    if B.ndim != 3 or y.shape != (B.shape[0],):
        raise ValueError("B is (rows, width, >= 3) and y_of_row has one entry per row")
    c = np.zeros(B.shape[:2], np.float32)
    with np.errstate(invalid="ignore"):
        h = np.abs(B[:, 1:] - B[:, :-1]).max(axis=-1)
        c[:, 1:] = np.maximum(c[:, 1:], h)
        c[:, :-1] = np.maximum(c[:, :-1], h)
        v = np.abs(B[1:] - B[:-1]).max(axis=-1)
        v = np.where((y[1:] == y[:-1] + 1)[:, None], v, np.float32(0))
        c[1:] = np.maximum(c[1:], v)
        c[:-1] = np.maximum(c[:-1], v)
    assert c.dtype == np.float32
    return c


def mask(B, y_of_row, threshold):
    """bool (rows, width): the refined pixels, !(contrast <= threshold); a NaN refines."""
    t = np.float32(threshold)
    if np.isnan(t):
        raise ValueError("the threshold is not NaN")
    with np.errstate(invalid="ignore"):
        return ~(contrast(B, y_of_row) <= t)


def near(B, y_of_row, threshold, eps=NEAR):
    """bool (rows, width): pixels whose contrast lies within eps of the threshold, so that frames
    differing by eps / 2 per channel may refine them or not."""
    with np.errstate(invalid="ignore"):
        return np.abs(contrast(B, y_of_row).astype(np.float64) - np.float64(threshold)) <= eps


def compose(B, S, m):
    """S where refined, B elsewhere."""
    B, S = np.asarray(B, np.float32), np.asarray(S, np.float32)
    if B.shape != S.shape or m.shape != B.shape[:2]:
        raise ValueError("B, S and the mask describe the same pixels")
    return np.where(m[..., None], S, B)
