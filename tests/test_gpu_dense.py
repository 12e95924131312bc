"""esl_dense_* on the device against its numpy statement (tests/dense_ref.py).

The comparison is exact: integers and the bytes of xyz alike.  Every scene is first checked, on the reference alone, for the conditions
that make this a fair demand (dense_scenes.check_conditions: no sample within 1e-9 of a voxel boundary, no fixed-point term within 1e-5
of a rounding tie); the reference of a scene is computed once and shared."""
import ctypes
import functools
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dense_ref as dr          # noqa: E402
import dense_scenes as sc       # noqa: E402

pytestmark = pytest.mark.gpu

OUTS = ("key", "xyz", "count", "bgr", "inst", "votes")
DTYPES = dict(key=np.int32, xyz=np.float64, count=np.int32, bgr=np.uint8, inst=np.int32, votes=np.int32)
MAXV = 65536          # the tests' default capacity: small tables
POS_SHIFT = (10.0, 10.0, 10.0)          # the whole room inside the voxel [0, 50)^3 of leaf 50


@functools.lru_cache(maxsize=None)
def room(seed=0, rows=sc.ROWS, cols=sc.COLS, shift=None):
    K = (60.0, 60.0, (cols - 1) / 2 + 0.25, (rows - 1) / 2 + 0.3) if (rows, cols) != (sc.ROWS, sc.COLS) else sc.K
    return sc.room_scene(seed, rows=rows, cols=cols, Kx=K, shift=shift)


@functools.lru_cache(maxsize=None)
def room_ref(seed, leaf, stride, shift=None):
    m, adds = sc.reference(room(seed, shift=shift), leaf=leaf, stride=stride, max_voxels=MAXV)
    sc.check_conditions(m, min_largest=100 if (leaf, stride) == (0.2, 1) else 0)
    return m, adds, m.extract()


def dev_add(cx, s, idx=None):
    idx = list(range(len(s["cams"]))) if idx is None else idx
    return cx.dense_add_frames(s["cams"][idx], s["K"], s["rows"], s["cols"], s["depth"][idx], s["bgr"][idx], s["inst"][idx])


def dev_map(pkg, cx, s, calls=None, with_color=True, with_inst=True, cap=None, want=OUTS, **over):
    over.setdefault("max_voxels", MAXV)
    cx.dense_begin(pkg.abi.default_dense_params(**over), with_color, with_inst)
    adds = [dev_add(cx, s, idx) for idx in (calls if calls is not None else [None])]
    return adds, cx.dense_info(), cx.dense_extract(cap, want)


def assert_map(dev, ref, keys=OUTS):
    assert dev["n_voxels"] == ref["n_voxels"]
    for k in keys:
        assert dev[k].dtype == DTYPES[k] and dev[k].shape == ref[k].shape, k
        if dev[k].tobytes() != ref[k].tobytes():
            bad = np.argwhere(np.asarray(dev[k]) != np.asarray(ref[k]))[:5]
            raise AssertionError((k, bad.tolist(), np.asarray(dev[k])[tuple(bad[0])], np.asarray(ref[k])[tuple(bad[0])]))


def same_bits(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.asarray(a[k]).tobytes() == np.asarray(b[k]).tobytes(), k


def check(pkg, cx, s, calls=None, with_color=True, with_inst=True, two_frames=True, **over):
    """device against the statement: the calls' counts, info and every output"""
    over.setdefault("max_voxels", MAXV)
    m, radds = sc.reference(s, calls, with_color, with_inst, **over)
    sc.check_conditions(m, two_frames=two_frames)
    adds, info, ext = dev_map(pkg, cx, s, calls, with_color, with_inst, **over)
    assert adds == radds and info == m.info()
    assert_map(ext, m.extract())
    return m, ext


# ---- scenes -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("stride", [1, 3])
@pytest.mark.parametrize("leaf", [0.01, 0.05, 0.2])
@pytest.mark.parametrize("seed", sc.ROOM_SEEDS)
def test_rooms(pkg, ctx, seed, leaf, stride):
    m, radds, ref = room_ref(seed, leaf, stride)
    adds, info, ext = dev_map(pkg, ctx, room(seed), leaf=leaf, stride=stride)
    assert adds == radds and info == m.info()
    assert_map(ext, ref)
    assert ext["n_voxels"] > 100 and (ext["inst"] >= 0).any() and ext["bgr"].any()


def test_one_voxel(pkg, ctx):
    """every sample on one slot: the contention case, and the run combine's longest run"""
    s = room(0, shift=POS_SHIFT)
    m, ext = check(pkg, ctx, s, leaf=50.0, depth_max=20.0)
    assert ext["n_voxels"] == 1 and ext["key"].tolist() == [[0, 0, 0]] and ext["count"][0] == m.info()["n_samples"] > 8000


@pytest.mark.parametrize("rows,cols", [(1, 65), (1, 129), (65, 1), (1, 1)])
@pytest.mark.parametrize("stride", [1, 3, 64])
def test_run_boundaries(pkg, ctx, rows, cols, stride):
    s = room(0, rows, cols)
    m, _ = check(pkg, ctx, s, leaf=0.05, stride=stride, two_frames=False)
    per = -(-rows // stride) * -(-cols // stride)
    assert m.info()["n_samples"] <= 3 * per and (m.info()["n_samples"] > 0 or per <= 2)


def test_nothing_to_add(pkg, ctx):
    s = dict(room(0))
    s["depth"] = np.zeros_like(s["depth"])
    adds, info, ext = dev_map(pkg, ctx, s)
    n = 3 * sc.ROWS * sc.COLS
    assert adds == [dict(n_sampled=n, n_zero=n, n_depth_out=0, n_key_out=0, n_used=0, status=0)]
    assert info["n_voxels"] == 0 and ext["n_voxels"] == 0 and all(len(ext[k]) == 0 for k in OUTS)
    s = room(0)
    adds, info, ext = dev_map(pkg, ctx, s, depth_min=5.0, depth_max=6.0)          # the room ends at about 2.5 m
    assert adds[0]["n_depth_out"] == n - adds[0]["n_zero"] > 8000 and adds[0]["n_used"] == 0 and ext["n_voxels"] == 0
    adds, info, ext = dev_map(pkg, ctx, s, depth_min=0.1, depth_max=0.5)
    assert adds[0]["n_depth_out"] == n - adds[0]["n_zero"] and ext["n_voxels"] == 0


def test_negative_and_far_keys(pkg, ctx):
    s = room(0, shift=sc.NEGATIVE_SHIFT)
    m, ext = check(pkg, ctx, s, leaf=0.05, depth_max=20.0)
    assert (ext["key"] < 0).all() and (ext["xyz"] < 0).all() and ext["n_voxels"] > 1000
    m, ext = check(pkg, ctx, room(0), leaf=1e-6, two_frames=False)          # 2 m / 1e-6 is beyond 2^20 - 1
    assert ext["n_voxels"] == 0 and m.info()["n_samples"] == 0
    adds = dev_map(pkg, ctx, room(0), leaf=1e-6)[0]
    assert adds[0]["n_key_out"] > 8000 and adds[0]["n_used"] == 0


def test_capacity(pkg, ctx):
    s = room(0)
    m, _, ref = room_ref(0, 0.2, 1)
    V = ref["n_voxels"]
    adds, info, ext = dev_map(pkg, ctx, s, leaf=0.2, max_voxels=V)
    assert adds[0]["status"] == 0 and info["status"] == 0
    assert_map(ext, ref)
    adds, info, ext = dev_map(pkg, ctx, s, leaf=0.2, max_voxels=V - 1)
    assert adds[0]["status"] == 3 and adds[0]["n_used"] == m.info()["n_samples"]
    assert info == dict(m.info(), n_voxels=-1, n_pairs=-1, status=3)
    assert ext["n_voxels"] == -1 and all(len(ext[k]) == 0 for k in OUTS)
    buf = {k: np.full((4,) + ((3,) if k in ("key", "xyz", "bgr") else ()), 77, DTYPES[k]) for k in OUTS}          # extract writes nothing
    n = ctypes.c_int64(5)
    L = pkg.lib.load()
    rc = L.esl_dense_extract(ctx._h, 4, *[buf[k].ctypes.data_as(t) for k, t in zip(OUTS, L.esl_dense_extract.argtypes[2:8])], ctypes.byref(n))
    assert rc == 0 and n.value == -1 and all((buf[k] == 77).all() for k in OUTS)
    again = dev_add(ctx, s)          # a further add: ESL_OK, nothing added
    assert again == dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0, status=3) and ctx.dense_info() == info
    # after esl_dense_begin the context works again
    adds, info, ext = dev_map(pkg, ctx, s, leaf=0.2)
    assert info["status"] == 0
    assert_map(ext, ref)
    # one voxel fits max_voxels = 1
    one = room(0, shift=POS_SHIFT)
    lab = dict(one, inst=np.where(one["inst"] >= 10, 1, np.where(one["inst"] >= 0, 0, -1)).astype(np.int32))          # two ids: two pairs
    mref, _ = sc.reference(lab, leaf=50.0, depth_max=20.0, max_voxels=1)
    adds, info, ext = dev_map(pkg, ctx, lab, leaf=50.0, depth_max=20.0, max_voxels=1)
    assert info == mref.info() and info["status"] == 0 and info["n_voxels"] == 1 and info["n_pairs"] == 2
    assert_map(ext, mref.extract())
    # ... but the room's six ids on it are more than 2 max_voxels pairs
    mref, _ = sc.reference(one, leaf=50.0, depth_max=20.0, max_voxels=1)
    assert mref.status == 3 and mref.n_voxels() == 1 and mref.n_pairs() == 6
    adds, info, ext = dev_map(pkg, ctx, one, leaf=50.0, depth_max=20.0, max_voxels=1)
    assert adds[0]["status"] == 3 and info == mref.info() and ext["n_voxels"] == -1
    assert dev_map(pkg, ctx, one, leaf=50.0, depth_max=20.0, max_voxels=3)[1]["status"] == 0


def test_incremental_equals_batch_equals_repeat(pkg, ctx):
    s = room(1)
    _, _, ref = room_ref(1, 0.05, 1)
    batch = dev_map(pkg, ctx, s, leaf=0.05)[2]
    assert_map(batch, ref)
    same_bits(batch, dev_map(pkg, ctx, s, calls=[[0], [1], [2]], leaf=0.05)[2])
    same_bits(batch, dev_map(pkg, ctx, s, calls=[[2], [1], [0]], leaf=0.05)[2])
    same_bits(batch, dev_map(pkg, ctx, s, calls=[[2, 1, 0]], leaf=0.05)[2])
    # an extract between adds changes nothing
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=0.05, max_voxels=MAXV))
    dev_add(ctx, s, [0])
    part = ctx.dense_extract()
    assert_map(part, sc.reference(s, [[0]], leaf=0.05)[0].extract())
    same_bits(part, ctx.dense_extract())
    dev_add(ctx, s, [1, 2])
    same_bits(batch, ctx.dense_extract())
    # fresh contexts
    runs = []
    for _ in range(2):
        cx = pkg.Context(0)
        try:
            runs.append(dev_map(pkg, cx, s, leaf=0.05)[2])
        finally:
            cx.close()
    same_bits(runs[0], runs[1]); same_bits(runs[0], batch)


def test_plain_and_combined_insert_agree(pkg, ctx):
    """ESL_DENSE_COMBINE picks the insert kernel's form at esl_dense_begin: integer sums, the same bits"""
    old = os.environ.get("ESL_DENSE_COMBINE")
    res = {}
    try:
        for form in ("0", "1"):
            os.environ["ESL_DENSE_COMBINE"] = form
            res[form] = [dev_map(pkg, ctx, room(0), leaf=leaf)[2] for leaf in (0.01, 0.2)] + [dev_map(pkg, ctx, room(0, shift=POS_SHIFT), leaf=50.0, depth_max=20.0)[2]]
    finally:
        if old is None:
            os.environ.pop("ESL_DENSE_COMBINE", None)
        else:
            os.environ["ESL_DENSE_COMBINE"] = old
    for a, b in zip(res["0"], res["1"]):
        same_bits(a, b)
    assert_map(res["0"][0], room_ref(0, 0.01, 1)[2]); assert_map(res["0"][1], room_ref(0, 0.2, 1)[2])


def test_mixed_shapes(pkg, ctx):
    a, b = room(0), room(2, 31, 45)
    m = dr.DenseMap(leaf=0.05, max_voxels=MAXV)
    ra = [m.add_frames(x["cams"], x["K"], x["rows"], x["cols"], x["depth"], x["bgr"], x["inst"]) for x in (a, b)]
    sc.check_conditions(m)
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=0.05, max_voxels=MAXV))
    assert [dev_add(ctx, a), dev_add(ctx, b)] == ra and ctx.dense_info() == m.info()
    assert_map(ctx.dense_extract(), m.extract())


def test_cap(pkg, ctx):
    _, _, ref = room_ref(0, 0.05, 1)
    V = ref["n_voxels"]
    for cap in (0, V // 2, V + 10):
        ext = dev_map(pkg, ctx, room(0), leaf=0.05, cap=cap)[2]
        n = min(cap, V)
        assert ext["n_voxels"] == V and all(len(ext[k]) == n for k in OUTS)
        assert_map(ext, dict({k: ref[k][:n] for k in OUTS}, n_voxels=V))
    # the rows past the first cap stay as they were
    L = pkg.lib.load()
    key = np.full((V, 3), 77, np.int32); n = ctypes.c_int64(0)
    assert L.esl_dense_extract(ctx._h, V // 2, key.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None, None, None, None, None, ctypes.byref(n)) == 0
    assert n.value == V and np.array_equal(key[:V // 2], ref["key"][:V // 2]) and (key[V // 2:] == 77).all()


def test_optional_inputs_and_outputs(pkg, ctx):
    s = room(0)
    for wc in (False, True):
        for wi in (False, True):
            m, ext = check(pkg, ctx, s, with_color=wc, with_inst=wi, leaf=0.05)
            assert ext["bgr"].any() == wc and (ext["inst"] >= 0).any() == wi
    _, _, ref = room_ref(0, 0.05, 1)
    for k in OUTS:          # each output alone, and all but it
        ext = dev_map(pkg, ctx, s, leaf=0.05, want=(k,))[2]
        assert set(ext) == {k, "n_voxels"}
        assert_map(ext, ref, (k,))
        rest = tuple(o for o in OUTS if o != k)
        assert_map(dev_map(pkg, ctx, s, leaf=0.05, want=rest)[2], ref, rest)
    assert dev_map(pkg, ctx, s, leaf=0.05, want=())[2] == dict(n_voxels=ref["n_voxels"])
    # bgr and inst passed but not asked for are not read: one-byte buffers
    ctx.dense_begin(pkg.abi.default_dense_params(leaf=0.05, max_voxels=MAXV), False, False)
    raw_add(pkg, ctx, s, bgr=np.zeros(1, np.uint8), inst=np.zeros(1, np.int32))
    assert_map(ctx.dense_extract(), sc.reference(s, with_color=False, with_inst=False, leaf=0.05)[0].extract())


def raw_add(pkg, cx, s, ctx_h=True, **over):
    """the C-ABI itself, every argument free; raises like the binding.  Arrays are passed flat, without a shape check."""
    L = pkg.lib.load()
    a = dict(cams=s["cams"], F=len(s["cams"]), K=s["K"], rows=s["rows"], cols=s["cols"], depth=s["depth"], bgr=s["bgr"], inst=s["inst"])
    a.update(over)
    keep = []

    def arr(x, dt, t):
        if x is None:
            return None
        x = np.ascontiguousarray(x, dtype=dt); keep.append(x)
        return x.ctypes.data_as(ctypes.POINTER(t))
    res = pkg.abi.EslDenseAddResult()
    rc = L.esl_dense_add_frames(cx._h if ctx_h else None, arr(a["cams"], np.float64, ctypes.c_double), a["F"], arr(a["K"], np.float64, ctypes.c_double),
                                a["rows"], a["cols"], arr(a["depth"], np.uint16, ctypes.c_uint16), arr(a["bgr"], np.uint8, ctypes.c_uint8),
                                arr(a["inst"], np.int32, ctypes.c_int32), ctypes.byref(res))
    if rc != 0:
        raise pkg.EslError(f"esl_dense_add_frames failed with esl_status {rc}: {L.esl_last_error().decode()}")
    return res.as_dict()


# ---- the resident cameras -----------------------------------------------------------------------------------------------------------------------------
def test_resident_cameras(pkg):
    g, c, o, _ = pkg.synth.make_graph(12, 30, 200, seed=3)
    rng = np.random.default_rng(5)
    cx = pkg.Context(0)
    try:
        cx.upload_graph(g); cx.upload_states(c, o)
        c0, o0 = cx.download_states()
        F = len(c0)
        assert F == g.n_cams
        s = dict(cams=c0, K=(40.0, 40.0, 7.6, 5.3), rows=12, cols=16, depth=rng.integers(2600, 20000, (F, 12, 16)).astype(np.uint16),
                 bgr=rng.integers(0, 256, (F, 12, 16, 3), dtype=np.uint8), inst=rng.integers(-1, 4, (F, 12, 16)).astype(np.int32))
        given = dev_map(pkg, cx, s, leaf=0.05)[2]
        m, _ = sc.reference(s, leaf=0.05, max_voxels=MAXV)
        sc.check_conditions(m, two_frames=False)
        assert_map(given, m.extract())
        cx.dense_begin(pkg.abi.default_dense_params(leaf=0.05, max_voxels=MAXV))
        cx.dense_add_frames(None, s["K"], 12, 16, s["depth"], s["bgr"], s["inst"])
        same_bits(given, cx.dense_extract())
        c1, o1 = cx.download_states()
        assert c0.tobytes() == c1.tobytes() and o0.tobytes() == o1.tobytes()
        info = cx.dense_info()
        with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_add_frames: F differs from the resident graph's n_cams"):
            raw_add(pkg, cx, s, cams=None, F=F - 1)
        assert cx.dense_info() == info
    finally:
        cx.close()


# ---- errors -----------------------------------------------------------------------------------------------------------------------------------------
def test_errors(pkg):
    s = room(0)
    cx = pkg.Context(0)
    P = pkg.abi.default_dense_params
    L = pkg.lib.load()
    nan, inf = float("nan"), float("inf")
    try:
        # before begin
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_add_frames: no esl_dense_begin"):
            raw_add(pkg, cx, s)
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_info_get"):
            cx.dense_info()
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_extract"):
            cx.dense_extract(4)
        cx.dense_end()          # nothing to forget: fine
        for bad, word in ((dict(leaf=0.0), "leaf"), (dict(leaf=-0.01), "leaf"), (dict(leaf=nan), "leaf"), (dict(leaf=inf), "leaf"),
                          (dict(depth_scale=0.0), "depth_scale"), (dict(depth_scale=nan), "depth_scale"), (dict(depth_scale=inf), "depth_scale"),
                          (dict(depth_min=nan), "depth_min"), (dict(depth_max=inf), "depth_max"), (dict(depth_min=3.0, depth_max=2.0), "depth_min > depth_max"),
                          (dict(stride=0), "stride"), (dict(stride=-2), "stride"), (dict(max_voxels=0), "max_voxels"),
                          (dict(max_voxels=(1 << 26) + 1), "max_voxels"), (dict(max_voxels=-1), "max_voxels")):
            with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_begin: .*" + word):
                cx.dense_begin(P(**bad))
        assert L.esl_dense_begin(None, None, 1, 1) == 2 and L.esl_dense_begin(cx._h, None, -1, 0) == 2 and L.esl_dense_begin(cx._h, None, 0, -1) == 2
        with pytest.raises(pkg.EslError, match="esl_status 4"):          # a refused begin starts nothing
            cx.dense_info()
        assert L.esl_dense_begin(cx._h, None, 1, 1) == 0          # NULL = defaults
        assert cx.dense_info() == dict(n_samples=0, n_voxels=0, n_pairs=0, status=0, with_color=1, with_inst=1)
        cx.dense_begin(P(leaf=0.05, max_voxels=MAXV))
        raw_add(pkg, cx, s, cams=s["cams"][:1], F=1, depth=s["depth"][:1], bgr=s["bgr"][:1], inst=s["inst"][:1])
        before, info = cx.dense_extract(), cx.dense_info()
        cases = [
            (dict(ctx_h=False), "ctx"), (dict(F=-1), "F"), (dict(K=None), "K"), (dict(depth=None), "depth"),
            (dict(rows=0), "rows"), (dict(rows=16385), "rows"), (dict(rows=-3), "rows"), (dict(cols=0), "cols"), (dict(cols=16385), "cols"),
            (dict(K=(0.0, 60, 4, 4)), "fx"), (dict(K=(nan, 60, 4, 4)), "fx"), (dict(K=(inf, 60, 4, 4)), "fx"), (dict(K=(-60.0, 60, 4, 4)), "fx"),
            (dict(K=(60, 0.0, 4, 4)), "fy"), (dict(K=(60, nan, 4, 4)), "fy"), (dict(K=(60, -1.0, 4, 4)), "fy"),
        ]
        for k, v in ((1, nan), (4, inf), (0, -inf)):          # an invalid pose in frame 2 of 3
            cams = s["cams"].copy(); cams[1, k] = v
            cases.append((dict(cams=cams), "pose"))
        cams = s["cams"].copy(); cams[1, 3:] = 0.0
        cases.append((dict(cams=cams), "pose"))
        cams = s["cams"].copy(); cams[1, 3:] = 1e200          # the norm overflows
        cases.append((dict(cams=cams), "pose"))
        for over, word in cases:
            with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_add_frames: .*" + word):
                raw_add(pkg, cx, s, **over)
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_add_frames: .*bgr"):
            raw_add(pkg, cx, s, bgr=None)
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_add_frames: .*inst"):
            raw_add(pkg, cx, s, inst=None)
        with pytest.raises(pkg.EslError, match="esl_status 4: esl_dense_add_frames: NULL cams needs a resident graph with states"):
            raw_add(pkg, cx, s, cams=None)
        # n_samples may not reach 2^31: a frame claimed to be 16384 x 16384, eight of them (nothing of it is read before the refusal)
        with pytest.raises(pkg.EslError, match="esl_status 2: esl_dense_add_frames: .*2\\^31"):
            raw_add(pkg, cx, s, cams=np.tile(s["cams"][:1], (8, 1)), F=8, rows=16384, cols=16384)
        n = ctypes.c_int64(0)
        assert L.esl_dense_extract(cx._h, -1, None, None, None, None, None, None, ctypes.byref(n)) == 2
        assert L.esl_dense_extract(cx._h, 4, None, None, None, None, None, None, None) == 2
        assert L.esl_dense_extract(None, 4, None, None, None, None, None, None, ctypes.byref(n)) == 2
        assert L.esl_dense_info_get(cx._h, None) == 2 and L.esl_dense_info_get(None, ctypes.byref(pkg.abi.EslDenseInfo())) == 2
        assert L.esl_dense_end(None) == 2 and L.esl_debug_dense_allocs(cx._h, None, None) == 2
        # every refused call left the map as it was
        assert cx.dense_info() == info
        same_bits(before, cx.dense_extract())
        # valid all the same
        assert raw_add(pkg, cx, s, cams=None, F=0, depth=None, bgr=None, inst=None)["n_sampled"] == 0
        assert raw_add(pkg, cx, s, cams=np.zeros((0, 7)), F=0)["n_sampled"] == 0
        assert cx.dense_info() == info
        assert L.esl_dense_add_frames(cx._h, s["cams"][1:].ctypes.data_as(ctypes.POINTER(ctypes.c_double)), 2,
                                      np.asarray(s["K"], np.float64).ctypes.data_as(ctypes.POINTER(ctypes.c_double)), s["rows"], s["cols"],
                                      s["depth"][1:].ctypes.data_as(ctypes.POINTER(ctypes.c_uint16)),
                                      s["bgr"][1:].ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
                                      s["inst"][1:].ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), None) == 0          # out may be NULL
        assert_map(cx.dense_extract(), room_ref(0, 0.05, 1)[2])
        cx.dense_end()
        with pytest.raises(pkg.EslError, match="esl_status 4"):
            cx.dense_extract(4)
        # the binding's own checks
        cx.dense_begin(P(leaf=0.05, max_voxels=MAXV))
        with pytest.raises(ValueError):
            cx.dense_add_frames(s["cams"], s["K"], s["rows"], s["cols"] + 1, s["depth"], s["bgr"], s["inst"])
        with pytest.raises(ValueError):
            cx.dense_extract(want=("colour",))
    finally:
        cx.close()


# ---- repeats and buffers ----------------------------------------------------------------------------------------------------------------------------
def test_grow_only_buffers(pkg):
    big, small = room(0), room(2, 31, 45)
    cx = pkg.Context(0)
    try:
        assert cx.dense_allocs() == (0, 0)
        a0 = dev_map(pkg, cx, big, leaf=0.01)[2]
        allocs = cx.dense_allocs()
        assert allocs[0] > 0 and allocs[1] > 0
        a1 = dev_map(pkg, cx, big, leaf=0.01)[2]          # warm: the largest scene again
        assert cx.dense_allocs() == allocs
        same_bits(a0, a1)
        assert_map(a1, room_ref(0, 0.01, 1)[2])
        check(pkg, cx, small, leaf=0.05)          # a smaller scene after a larger one reads nothing the larger one left behind
        check(pkg, cx, big, calls=[[0], [1, 2]], leaf=0.2, with_color=False)
        assert cx.dense_allocs() == allocs
        for owner in cx.SCRATCH_OWNERS:
            assert cx.scratch_allocs(owner) == (0, 0), owner
    finally:
        cx.close()


def test_default_capacity(pkg):
    cx = pkg.Context(0)
    try:
        cx.dense_begin()          # the defaults: leaf 0.01, 2^20 voxels
        assert dev_add(cx, room(0)) == room_ref(0, 0.01, 1)[1][0]
        assert_map(cx.dense_extract(), room_ref(0, 0.01, 1)[2])
    finally:
        cx.close()


def test_profiling_class_4(pkg):
    cx = pkg.Context(0)
    try:
        cx.profile_enable(2)
        dev_map(pkg, cx, room(0), leaf=0.05)
        prof = cx.profile_get()
        assert set(prof) == {"reduce"} and prof["reduce"]["count"] >= 2 and prof["reduce"]["total_ms"] > 0
    finally:
        cx.close()


# ---- the refusal ladder: every argument wrong at once, repaired one rung at a time, in the entry's order ----------------------------------------
def test_add_frames_refusal_ladder(pkg):
    """esl_dense_add_frames with every argument wrong at once: the status and the whole text of the first refusal, that argument repaired,
    the next refusal, through the entry's sequence.  No map until "no esl_dense_begin before" has come out, then a map of one 4 x 4
    frame; nothing is added until the last call, which adds that frame again."""
    who = "esl_dense_add_frames"
    good = np.array([[0, 0, 0, 0, 0, 0, 1.0]] * 8)
    bad = good.copy(); bad[5, 3:] = 0
    depth, bgr, inst = np.full((1, 4, 4), 5000, np.uint16), np.full((1, 4, 4, 3), 9, np.uint8), np.zeros((1, 4, 4), np.int32)
    K = (60.0, 60.0, 1.5, 1.5)
    one = dict(cams=good[:1], K=K, rows=4, cols=4, depth=depth, bgr=bgr, inst=inst)
    a = dict(ctx_h=False, cams=None, F=-1, K=None, rows=0, cols=16385, depth=None, bgr=None, inst=None)          # every argument wrong
    ladder = [          # (status, text, the repair); rows = cols = 16384 and F = 8 are valid and hold 2^31 samples
        (2, "null ctx", dict(ctx_h=True)),
        (2, "negative F", dict(F=8)),
        (2, "null K", dict(K=(0.0, np.inf, 1.5, 1.5))),
        (2, "rows < 1 or > 16384", dict(rows=16384)),
        (2, "cols < 1 or > 16384", dict(cols=16384)),
        (2, "fx not finite or <= 0", dict(K=(60.0, np.inf, 1.5, 1.5))),
        (2, "fy not finite or <= 0", dict(K=K)),
        (2, "null depth", dict(depth=depth)),
        (4, "no esl_dense_begin before", "map"),
        (4, "null bgr on a map begun with colour", dict(bgr=bgr)),
        (4, "null inst on a map begun with labels", dict(inst=inst)),
        (4, "NULL cams needs a resident graph with states", dict(cams=bad)),
        (2, "a pose with a non-finite number or a quaternion of norm 0", dict(cams=good)),
        (2, "n_samples would reach 2^31", dict(rows=4, cols=4, F=1)),
    ]
    cx = pkg.Context(0)
    try:
        for status, text, repair in ladder:
            with pytest.raises(pkg.EslError) as e:
                raw_add(pkg, cx, one, **a)
            assert str(e.value) == f"{who} failed with esl_status {status}: {who}: {text}"
            if repair == "map":
                cx.dense_begin()
                cx.dense_add_frames(**one)
                before = cx.dense_info()
                assert before["n_samples"] == 16 and before["status"] == 0
            else:
                a.update(repair)
        assert cx.dense_info() == before          # every refused call left the map alone
        assert raw_add(pkg, cx, one, **a)["n_used"] == 16 and cx.dense_info()["n_samples"] == 32
    finally:
        cx.close()
