"""Built scenes for the single-frame fit (esl_fit_frame): small depth images whose stage counters are known by
construction, one per clustering substrate, hand-over and discrete decision of the fit.  numpy only, deterministic, reads
nothing.  tests/test_fit_scenes.py checks every scene's premise against the CPU checker and oracle/np_fit.py.  The scenes are
inputs for esl_fit_frame on the device as they stand (every box is a legal input); a device test over them is not in the
suite yet.

scene(name) -> Scene(depth u16 (h, w), boxes (B, 4), labels (B,), Twc (7,), intr (5,), ground (4,), params), `params` being
the overrides of the default fit parameters (a dict for default_fit_params(**params)).

Base construction: 640 x 480 image, intr = (500, 500, 320.5, 240.5, 5000) -- the half-pixel principal point keeps every
sample off the voxel borders --, identity pose, ground = (0, 0, 1, 10) so that the supporting-plane filter keeps everything,
and a slanted wall z = 2.0 + 0.15 (u - w/2)/w + 0.07 (v - h/2)/h.  At stride 3 the lateral pitch (12 mm at 2 m) exceeds the
10 mm voxel leaf: every in-range sample is its own voxel, M = number of samples, and one zeroed pixel removes exactly one.
"""
import collections

import numpy as np

Scene = collections.namedtuple("Scene", "depth boxes labels Twc intr ground params")

W, H = 640, 480
INTR = (500.0, 500.0, 320.5, 240.5, 5000.0)
TWC = (0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 1.0)
GROUND = (0.0, 0.0, 1.0, 10.0)

BOX_2048 = (100, 200, 292, 296)      # 64 x 32 samples at stride 3
BOX_2050 = (100, 100, 175, 346)      # 25 x 82
BOX_1024 = (100, 100, 148, 292)      # 16 x 64
BOX_1025 = (100, 100, 175, 223)      # 25 x 41
BOX_BIG = (10, 100, 430, 400)        # 140 x 100: workspace capacity 16384 > 8192, the frame goes grid-wide


def wall(z0=2.0, w=W, h=H):
    u, v = np.meshgrid(np.arange(w), np.arange(h))
    z = z0 + 0.15 * (u - w / 2) / w + 0.07 * (v - h / 2) / h
    return np.rint(z * INTR[4]).astype(np.uint16)


def patches(*specs, w=W, h=H):
    """zero image with rectangles (row0, row1, col0, col1, z0) of the slanted wall at depth z0"""
    d = np.zeros((h, w), dtype=np.uint16)
    for r0, r1, c0, c1, z0 in specs:
        d[r0:r1, c0:c1] = wall(z0, w, h)[r0:r1, c0:c1]
    return d


def centre_pixels(box):
    """the 10 x 10 pixels GetCenter samples (reference src/pca/EllipsoidExtractor.cpp:583-614)"""
    x, y = int((box[0] + box[2]) / 2.0), int((box[1] + box[3]) / 2.0)
    xd, yd = int(abs(box[0] - box[2]) / 4.0 / 10), int(abs(box[1] - box[3]) / 4.0 / 10)
    return [(x + i * xd, y + j * yd) for i in range(-5, 5) for j in range(-5, 5)]


def on_grid(box, stride, x, y):
    """is pixel (x, y) one of the box's scan samples"""
    x1, y1, x2, y2 = [int(v) for v in box]
    return x1 <= x < x2 and y1 <= y < y2 and (x - x1) % stride == 0 and (y - y1) % stride == 0


def _scene(depth, boxes, labels=None, intr=INTR, **params):
    boxes = np.asarray(boxes, dtype=np.float64).reshape(-1, 4)
    labels = np.zeros(len(boxes), np.int32) if labels is None else np.asarray(labels, dtype=np.int32)
    return Scene(np.ascontiguousarray(depth, dtype=np.uint16), boxes, labels, np.array(TWC), np.array(intr, dtype=np.float64),
                 np.array(GROUND), dict(params))


def _holes(d, box, n, stride=3):
    """zero n of the box's scan samples (away from the box centre's 10 x 10 patch)"""
    x1, y1 = int(box[0]), int(box[1])
    for k in range(n):
        d[y1 + stride * (2 + k), x1 + stride * (3 + 2 * k)] = 0
    return d


def _far_centre(d, box, z=1.0, stride=3):
    """Give GetCenter a centre the clusters do not contain: the centre pixels the scan does not sample get depth z, those it
    does sample get none.  The scan never sees the former, so the clusters are those of the patches alone."""
    n = 0
    for x, y in centre_pixels(box):
        if on_grid(box, stride, x, y):
            d[y, x] = 0
        else:
            d[y, x] = int(round(z * INTR[4])); n += 1
    assert n >= 2
    return d


# ---- substrate hand-overs -------------------------------------------------------------------------------------------
def _m(box, holes, **kw):
    return lambda: _scene(_holes(wall(), box, holes), [box], **kw)


# the wall's near patch of the mixed frame: box SMALL[2] sees it in front of the wall
def _mixed_depth():
    d = wall()
    d[300:345, 480:555] = wall(1.3)[300:345, 480:555]
    return d


SMALL = [BOX_2048, BOX_1024, (460, 280, 580, 380), (700, 100, 800, 200), (400, 50, 520, 110)]
SMALL_LABELS = [0, 41, 28, 0, 0]


def _strip():
    """One row of 1,200 connected samples, 1.12 m long at a cluster tolerance of 1 mm: more than 1,020 cells along x although
    M <= 2048.  Bowed and tilted in depth (less than one depth quantum per pixel) so that the PCA has three distinct axes."""
    w, h, fx = 1280, 64, 1070.0
    t = (np.arange(w) - 640.0) / 640.0
    z = 1.0 - 0.03 * t * t - 0.02 * t
    d = np.zeros((h, w), dtype=np.uint16)
    d[:, :] = np.rint(z * INTR[4]).astype(np.uint16)[None, :]
    return _scene(d, [(40, 32, 1240, 33)], intr=(fx, fx, 640.5, 32.5, 5000.0), stride=1, voxel_leaf=0.0005, cluster_tolerance=0.001)


BRIDGE_TOL = 0.075
BRIDGE_ROWS = (19, 13, 7, 26)


def bridge_sample(k):
    """(column, row), in samples of BOX_2048, of the two ends of bridge k"""
    return (14 * k + 7, BRIDGE_ROWS[k]), (14 * k + 13, BRIDGE_ROWS[k])


def _bridges():
    """Five blobs of 8 x 32 samples, 6 empty sample columns (7 pitches = 83 mm > tolerance) between neighbours, and ONE pair
    of points within the tolerance across each gap: a spur in the gap's last column, 6 pitches = 71 mm from the blob on its
    left, whose edge column is emptied two rows up and down so that no second pair reaches across.  The blobs form one
    cluster only if every one of the four pairs is linked -- and the point that records a pair has about 30 neighbours to
    record (tests/test_fit_scenes.py), twice a neighbour strip."""
    d0 = wall()
    d = d0.copy()
    x1, y1 = BOX_2048[0], BOX_2048[1]
    for k in range(4):
        d[y1:BOX_2048[3], x1 + 3 * (14 * k + 8):x1 + 3 * (14 * k + 14)] = 0
        (ci, r), (si, _) = bridge_sample(k)
        d[y1 + 3 * r, x1 + 3 * si] = d0[y1 + 3 * r, x1 + 3 * si]
        for dr in (-2, -1, 1, 2):
            d[y1 + 3 * (r + dr), x1 + 3 * ci] = 0
    return _scene(d, [BOX_2048], cluster_tolerance=BRIDGE_TOL)


# ---- cluster choice -------------------------------------------------------------------------------------------------
CH_SMALL_BOX = (50, 90, 390, 230)
CH_SMALL_FAR = (110, 200, 60, 180, 2.5)      # 30 x 40 samples
CH_SMALL_NEAR = (140, 185, 190, 280, 1.5)    # 15 x 30 samples, under the box centre
CH_SMALL_OTHER = (110, 200, 270, 340, 2.5)
CH_MID_BOX = (50, 90, 282, 335)              # 2,250 + ~400 points, capacity 8192: global memory inside the box's workgroup
CH_MID_FAR = (100, 325, 60, 150, 2.5)        # 75 x 30 samples
CH_MID_NEAR = (175, 250, 160, 214, 1.5)      # 25 x 18 samples
CH_LARGE_BOX = (50, 90, 650, 410)            # overhangs the image's right side; capacity 32768
CH_LARGE_FAR = (100, 400, 60, 300, 2.5)      # 100 x 80 samples
CH_LARGE_NEAR = (210, 290, 330, 450, 1.5)
CH_LARGE_FAR_NARROW = (100, 400, 60, 270, 2.5)
CH_LARGE_OTHER = (100, 400, 430, 610, 2.5)

TIE_SMALL_BOX = (97, 97, 280, 190)
TIE_SMALL_A = (100, 175, 112, 160, 2.0)      # 25 x 16 samples, the nearer patch: it holds the smaller voxel key
TIE_SMALL_B = (130, 178, 190, 265, 2.1)      # 16 x 25 samples, under the box centre
TIE_LARGE_BOX = (58, 97, 500, 380)
TIE_LARGE_A = (100, 370, 60, 210, 2.0)       # 90 x 50
TIE_LARGE_B = (100, 325, 250, 430, 2.1)      # 75 x 60


def _box_of(p, pad=3):
    """a box of its own around patch p whose scan grid is the grid of the tie boxes (origin = (58, 97) mod 3)"""
    r0, r1, c0, c1, _ = p
    x1 = c0 - pad; x1 -= (x1 - 58) % 3
    y1 = r0 - pad; y1 -= (y1 - 97) % 3
    return (x1, y1, c1 + pad, r1 + pad)


# ---- centre patch ---------------------------------------------------------------------------------------------------
def _centre(n_valid):
    d0 = wall()
    d = d0.copy()
    d[230:262, 170:222] = 0
    for x, y in centre_pixels(BOX_2048)[:n_valid]:
        d[y, x] = d0[y, x]
    return _scene(d, [BOX_2048])


# ---- geometry and range edges ---------------------------------------------------------------------------------------
OVERHANG = [(-30.0, 100.0, 90.0, 250.0), (100.0, -25.0, 200.0, 80.0), (560.0, 100.0, 700.0, 220.0), (100.0, 400.0, 220.0, 520.0),
            (-3.7, -2.2, 120.6, 90.4),            # negative and fractional corners
            (-100.0, 100.0, 140.0, 190.0),        # part of the centre patch lies left of the image
            (-200.0, 100.0, 120.0, 220.0),        # all of it: status 1
            (500.3, 380.9, 655.5, 493.1)]         # two sides at once
DEGENERATE = [(300.0, 100.0, 200.0, 200.0), (100.0, 300.0, 200.0, 200.0), (100.0, 100.0, 100.0, 200.0), (100.0, 100.0, 200.0, 100.0),
              (700.0, 100.0, 800.0, 200.0), (-300.0, -300.0, -100.0, -100.0), (100.0, 480.0, 200.0, 600.0)]
BOX_STRIDE_A = (100, 100, 161, 189)     # 61 x 89 pixels: neither 2, 5 nor 7 divides either side
BOX_STRIDE_B = (100, 100, 403, 321)     # 303 x 221


def _depth_limits():
    d = wall()
    x1, y1 = BOX_2048[0], BOX_2048[1]
    for (i, j), v in {(2, 2): 500, (3, 2): 500, (4, 2): 500, (2, 4): 501, (3, 4): 501, (4, 4): 501, (10, 2): 30000, (11, 2): 30000,
                      (10, 4): 30001, (11, 4): 30001, (20, 2): 65535}.items():
        d[y1 + 3 * j, x1 + 3 * i] = v
    cx, cy = centre_pixels(BOX_2048)[55]      # the box centre, a scan sample too: 0.1 m exactly is out of the scan's range
    assert on_grid(BOX_2048, 3, cx, cy)       # (z <= depth_min in double) and inside GetCenter's (float 0.1f > 0.1)
    d[cy, cx] = 500
    return _scene(d, [BOX_2048])


def _depth_min_low():
    d = wall()
    x1, y1 = BOX_2048[0], BOX_2048[1]
    for i in range(2, 6):
        for j in range(2, 6):
            d[y1 + 3 * j, x1 + 3 * i] = 400   # 0.08 m: inside the scan's range once depth_min = 0.05, never inside GetCenter's 0.1
    cx, cy = centre_pixels(BOX_2048)[55]
    d[cy, cx] = 400
    return _scene(d, [BOX_2048], depth_min=0.05)


_BUILDERS = {
    # M = samples = voxels: 2048 is the last size of the LDS clustering
    "m2047": _m(BOX_2048, 1), "m2048": _m(BOX_2048, 0), "m2049": _m(BOX_2050, 1), "m2048_pair": _m(BOX_2050, 2),
    "m2050": _m(BOX_2050, 0),
    # chosen cluster of 1024 / 1025 voxels with a symmetry label: 1024 is the last size of the LDS symmetry grid
    "nc1024": lambda: _scene(wall(), [BOX_1024], [41]), "nc1024_dual": lambda: _scene(wall(), [BOX_1024], [28]),
    "nc1025": lambda: _scene(wall(), [BOX_1025], [41]),
    "strip_extent": _strip,
    # ~30 neighbours per point in the half space the search visits: the 16-entry neighbour strip overflows
    "m2048_tol50": lambda: _scene(wall(), [BOX_2048], cluster_tolerance=0.05),
    # the same overflow where one lost neighbour splits the cluster
    "tol75_bridges": _bridges,
    "mixed": lambda: _scene(_mixed_depth(), [BOX_BIG] + SMALL, [0] + SMALL_LABELS),
    "mixed_small_only": lambda: _scene(_mixed_depth(), SMALL, SMALL_LABELS),
    # two clusters, the smaller one near the centre: center_dis 0.5 takes it, center_dis 5 takes the larger
    "choice_near_small": lambda: _scene(patches(CH_SMALL_FAR, CH_SMALL_NEAR), [CH_SMALL_BOX], center_dis=0.5),
    "choice_largest_small": lambda: _scene(patches(CH_SMALL_FAR, CH_SMALL_NEAR), [CH_SMALL_BOX], center_dis=5.0),
    "choice_near_global": lambda: _scene(patches(CH_MID_FAR, CH_MID_NEAR), [CH_MID_BOX], center_dis=0.5),
    "choice_largest_global": lambda: _scene(patches(CH_MID_FAR, CH_MID_NEAR), [CH_MID_BOX], center_dis=5.0),
    "choice_near_large": lambda: _scene(patches(CH_LARGE_FAR, CH_LARGE_NEAR), [CH_LARGE_BOX], center_dis=0.5),
    "choice_largest_large": lambda: _scene(patches(CH_LARGE_FAR, CH_LARGE_NEAR), [CH_LARGE_BOX], center_dis=5.0),
    # a lone cluster is taken however far from the centre; with a second one beside it nothing is within center_dis
    "choice_lone_small": lambda: _scene(_far_centre(patches(CH_SMALL_FAR), CH_SMALL_BOX), [CH_SMALL_BOX]),
    "choice_none_small": lambda: _scene(_far_centre(patches(CH_SMALL_FAR, CH_SMALL_OTHER), CH_SMALL_BOX), [CH_SMALL_BOX]),
    "choice_lone_large": lambda: _scene(_far_centre(patches(CH_LARGE_FAR_NARROW), CH_LARGE_BOX), [CH_LARGE_BOX]),
    "choice_none_large": lambda: _scene(_far_centre(patches(CH_LARGE_FAR_NARROW, CH_LARGE_OTHER), CH_LARGE_BOX), [CH_LARGE_BOX]),
    "choice_lone_tight": lambda: _scene(patches(CH_LARGE_FAR, CH_LARGE_NEAR), [(50, 90, 310, 410)], center_dis=0.01),
    # min_cluster_size at the cluster's size and one above it
    "minsize_eq_small": lambda: _scene(wall(), [BOX_2048], min_cluster_size=2048),
    "minsize_above_small": lambda: _scene(wall(), [BOX_2048], min_cluster_size=2049),
    "minsize_eq_large": lambda: _scene(wall(), [BOX_BIG], min_cluster_size=14000),
    "minsize_above_large": lambda: _scene(wall(), [BOX_BIG], min_cluster_size=14001),
    # two clusters of equal size, both within center_dis, a depth step of 0.1 m between them
    "tie_small": lambda: _scene(patches(TIE_SMALL_A, TIE_SMALL_B), [TIE_SMALL_BOX]),
    "tie_small_a": lambda: _scene(patches(TIE_SMALL_A, TIE_SMALL_B), [_box_of(TIE_SMALL_A)]),
    "tie_small_b": lambda: _scene(patches(TIE_SMALL_A, TIE_SMALL_B), [_box_of(TIE_SMALL_B)]),
    "tie_large": lambda: _scene(patches(TIE_LARGE_A, TIE_LARGE_B), [TIE_LARGE_BOX]),
    "tie_large_a": lambda: _scene(patches(TIE_LARGE_A, TIE_LARGE_B), [_box_of(TIE_LARGE_A)]),
    "tie_large_b": lambda: _scene(patches(TIE_LARGE_A, TIE_LARGE_B), [_box_of(TIE_LARGE_B)]),
    # valid samples in the centre patch: none, one (both status 1), two
    "centre_hole": lambda: _centre(0), "centre_one": lambda: _centre(1), "centre_two": lambda: _centre(2),
    "boxes_overhang": lambda: _scene(wall(), OVERHANG, [0, 41, 28, 0, 41, 0, 0, 28]),
    "boxes_degenerate": lambda: _scene(wall(), DEGENERATE),
    "stride1": lambda: _scene(wall(), [BOX_STRIDE_A], stride=1), "stride2": lambda: _scene(wall(), [BOX_STRIDE_A], stride=2),
    "stride5": lambda: _scene(wall(), [BOX_STRIDE_B], stride=5, cluster_tolerance=0.05),
    "stride7": lambda: _scene(wall(), [BOX_STRIDE_B], stride=7, cluster_tolerance=0.05),
    "depth_limits": _depth_limits, "depth_min_low": _depth_min_low,
    # corners near the +-1e6 limit: 267,520 scan positions, 856 of them inside the image
    "huge_box": lambda: _scene(wall(), [(-99999.3, 100.5, 100639.3, 112.9)]),
}
NAMES = tuple(_BUILDERS)
_cache = {}


def scene(name):
    if name not in _cache:
        s = _BUILDERS[name]()
        s.depth.setflags(write=False)
        _cache[name] = s
    return _cache[name]
