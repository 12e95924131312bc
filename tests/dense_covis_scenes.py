"""Scenes of the esl_dense_covis_frames tests, everything from fixed numbers.  dense_carve_scenes' rooms (`ghost`, `ghost_odd`, ...) and
point maps are reused as they are; added here: `away`, the room's six views plus three that look at the opposite corner, so that some
pairs of frames share no voxel; `hand`, three voxels at dyadic points and four identity-pose frames of 1 x 3 pixels whose bit matrix and
pair counts are written out; `points(n)`, n voxels in a row for the word boundaries; `cycled`, any number of frames from a scene's
views.  The CPU test asserts its premises on these, the GPU test runs them.  Nothing here is imported by the package."""
import functools

import numpy as np

import dense_align_scenes as das
import dense_carve_scenes as cs

AWAY_VIEWS = [((1.8, 1.4, 1.2), (3.9, 2.9, 2.3)), ((2.0, 1.2, 1.4), (3.8, 2.6, 0.2)), ((1.6, 1.7, 1.0), (3.9, 1.0, 2.4))]


@functools.lru_cache(maxsize=None)
def away(rows=45, cols=61):
    """the room without the box from nine views: dense_align_scenes.MAP_VIEWS look into the corner at LO, AWAY_VIEWS at the corner at HI"""
    s = cols / das.COLS
    Kx = (das.K[0] * s, das.K[1] * s, (cols - 1) / 2, (rows - 1) / 2)
    cams = np.stack([das.look_at(das.LO + np.array(o), das.LO + np.array(t)) for o, t in das.MAP_VIEWS + AWAY_VIEWS])
    depth = np.stack([das.box_depth(c, Kx, rows, cols) for c in cams])
    return dict(cams=cams, K=Kx, rows=rows, cols=cols, depth=depth, hit=None, bgr=None, inst=None, params=dict(das.MAP_PARAMS), with_color=False,
                with_inst=False)


def scene(name):
    return away() if name == "away" else cs.ghost_scene(name)


ROOMS = tuple(cs.GHOSTS) + ("away",)


def cycled(sc, F):
    """F frames from the scene's V views: frame j is view j % V; in every odd repetition an exact duplicate of the frame V before it,
    in every even one the view moved by 4 mm per repetition along the camera's x -> (cams (F, 7), depth (F, rows, cols))"""
    V = len(sc["cams"])
    cams = np.stack([sc["cams"][j % V] for j in range(F)]) if F else np.zeros((0, 7))
    for j in range(F):
        rep = j // V
        cams[j, 0] += 0.004 * (rep - rep % 2)
    depth = np.stack([sc["depth"][j % V] for j in range(F)]) if F else np.zeros((0, sc["rows"], sc["cols"]), np.uint16)
    return cams, depth


# ---- the hand-made scene: voxel j of the three is seen through pixel j of a 1 x 3 image -------------------------------------------------
HAND_POINTS = [(-1, 0, 1), (0, 0, 1), (1, 0, 1)]
A, Z, T_ = cs.A, cs.Z, cs.T_          # raw values that agree with z = 1, hold no data, lie beyond it
HAND_DEPTH = np.array([[[A, A, Z]], [[Z, A, A]], [[A, A, A]], [[T_, Z, T_]]], np.uint16)
HAND_B = [[1, 1, 0], [0, 1, 1], [1, 1, 1], [0, 0, 0]]          # per frame, per point of HAND_POINTS
HAND_K_COUNT = [2, 3, 2]                                        # per point
HAND_PAIR = [[2, 1, 2, 0],
             [1, 2, 2, 0],
             [2, 2, 3, 0],
             [0, 0, 0, 0]]
HAND_FRAME = [[3, 0, 0, 2, 1, 0, -1, 0],          # at min_others = 2: covered = the voxels whose k - 1 >= 2, i.e. the middle one
              [3, 0, 0, 2, 1, 0, -1, 0],
              [3, 0, 0, 3, 1, 0, -1, 0],
              [3, 0, 0, 0, 0, 0, -1, 0]]
HAND_PARAMS = dict(cs.EXACT_PARAMS, window=0, min_others=2)
HAND_PARAMS.pop("min_through")


@functools.lru_cache(maxsize=None)
def hand():
    fr = das.point_frames(HAND_POINTS)
    sc = dict(cams=fr["cams"], K=fr["K"], rows=fr["rows"], cols=fr["cols"], depth=fr["depth"], bgr=None, inst=None, hit=None,
              params=dict(cs.EXACT_MAP), with_color=False, with_inst=False)
    return dict(map=sc, cams=np.tile(np.array(cs.IDENT), (4, 1)), depth=HAND_DEPTH, K=(1.0, 1.0, 1.0, 0.0), rows=1, cols=3, params=dict(HAND_PARAMS))


def hand_order(m):
    """index of each of HAND_POINTS in m.extract()'s order"""
    index = {tuple(k): i for i, k in enumerate(m.extract()["key"].tolist())}
    return [index[tuple(int(np.floor(v / das.PLEAF)) for v in pt)] for pt in HAND_POINTS]


# ---- n voxels in a row: the word boundaries ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def points(n):
    """a map of n voxels at (j / 64 + 1 / 128, 0, 1), j < n, and three identity-pose frames of 1 x n pixels at fx = 64: voxel j projects
    to pixel j exactly.  Frame 0 agrees everywhere, frame 1 at the even pixels, frame 2 at pixel n - 1 and at every pixel 5 mod 7"""
    pts = [(j / 64 + 1 / 128, 0.0, 1.0) for j in range(n)]
    fr = das.point_frames(pts)
    sc = dict(cams=fr["cams"], K=fr["K"], rows=fr["rows"], cols=fr["cols"], depth=fr["depth"], bgr=None, inst=None, hit=None,
              params=dict(cs.EXACT_MAP), with_color=False, with_inst=False)
    j = np.arange(n)
    depth = np.stack([np.full(n, A), np.where(j % 2 == 0, A, Z), np.where((j == n - 1) | (j % 7 == 5), A, T_)]).astype(np.uint16).reshape(3, 1, n)
    B = np.stack([np.ones(n, bool), j % 2 == 0, (j == n - 1) | (j % 7 == 5)])
    return dict(map=sc, cams=np.tile(np.array(cs.IDENT), (3, 1)), depth=depth, K=(64.0, 1.0, -0.5, 0.0), rows=1, cols=n,
                params=dict(HAND_PARAMS, min_others=1), B=B)
