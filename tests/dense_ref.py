"""The numpy statement of esl_dense_* (include/esl.h, "the dense map", steps 1-7): every sample of every frame is kept as a row (packed
key, fixed-point terms, colour, id); a map is extracted with np.unique over the packed keys and int64 sums.  The arithmetic follows the
header operation by operation -- the device is compared with it exactly, bytes of xyz included -- so nothing here may be "simplified".
Test infrastructure only: nothing here is imported by the package."""
import numpy as np

DEFAULTS = dict(leaf=0.01, depth_scale=5000.0, depth_min=0.5, depth_max=6.0, stride=1, max_voxels=1048576)
KEY_OFF, KEY_MAX = 1 << 20, (1 << 20) - 1
FIX = float(1 << 30)


class InvalidPose(ValueError):
    pass


def pose(cam):
    """step 2 -> (R (3, 3), t (3,)) of a Tcw row (t, q); the operations in the header's order"""
    cam = [float(v) for v in cam]
    with np.errstate(all="ignore"):
        nrm = np.sqrt(np.float64(cam[3] * cam[3] + cam[4] * cam[4] + cam[5] * cam[5] + cam[6] * cam[6]))
    if not np.isfinite(cam).all() or not np.isfinite(nrm) or not nrm > 0:
        raise InvalidPose("a pose with a non-finite number or a quaternion of norm 0")
    nrm = float(nrm)
    x, y, z, w = cam[3] / nrm, cam[4] / nrm, cam[5] / nrm, cam[6] / nrm
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    R = np.array([[1 - (tyy + tzz), txy - twz, txz + twy],
                  [txy + twz, 1 - (txx + tzz), tyz - twx],
                  [txz - twy, tyz + twx, 1 - (txx + tyy)]])
    return R, np.array(cam[:3])


def pack(k):
    """(n, 3) integer keys -> uint64: the unsigned order is the lexicographic order of (kx, ky, kz)"""
    k = np.asarray(k, dtype=np.int64) + KEY_OFF
    return (k[..., 0].astype(np.uint64) << np.uint64(42)) | (k[..., 1].astype(np.uint64) << np.uint64(21)) | k[..., 2].astype(np.uint64)


def unpack(key):
    key = np.asarray(key, dtype=np.uint64)
    m = np.uint64(0x1FFFFF)
    return np.stack([(key >> np.uint64(42)) & m, (key >> np.uint64(21)) & m, key & m], axis=-1).astype(np.int64) - KEY_OFF


def samples(cam, K, rows, cols, depth, p):
    """steps 1-3 of one frame -> dict(row, col of the used samples, pw (n, 3), k (n, 3) int64, counts)"""
    fx, fy, cx, cy = (float(v) for v in K)
    st = int(p["stride"])
    rr_, cc = np.meshgrid(np.arange(0, rows, st), np.arange(0, cols, st), indexing="ij")
    rr_, cc = rr_.reshape(-1), cc.reshape(-1)
    raw = np.asarray(depth)[rr_, cc]
    counts = dict(n_sampled=int(raw.size), n_zero=int((raw == 0).sum()))
    z = raw.astype(np.float64) / p["depth_scale"]
    out = (raw != 0) & ((z < p["depth_min"]) | (z > p["depth_max"]))
    counts["n_depth_out"] = int(out.sum())
    ok = (raw != 0) & ~out
    rr_, cc, z = rr_[ok], cc[ok], z[ok]
    pc0 = (cc.astype(np.float64) - cx) * z / fx
    pc1 = (rr_.astype(np.float64) - cy) * z / fy
    R, t = pose(cam)
    d0, d1, d2 = pc0 - t[0], pc1 - t[1], z - t[2]
    pw = np.stack([(R[0, a] * d0 + R[1, a] * d1) + R[2, a] * d2 for a in range(3)], axis=-1)
    with np.errstate(all="ignore"):
        kf = np.floor(pw / p["leaf"])
    inr = (np.abs(kf) <= KEY_MAX).all(axis=-1)          # NaN and infinities compare false
    counts["n_key_out"] = int((~inr).sum())
    counts["n_used"] = int(inr.sum())
    return dict(row=rr_[inr], col=cc[inr], pw=pw[inr], k=kf[inr].astype(np.int64), counts=counts)


class DenseMap:
    """begin / add_frames / info / extract, as the C calls"""

    def __init__(self, with_color=True, with_inst=True, **over):
        self.p = dict(DEFAULTS); self.p.update(over)
        self.with_color, self.with_inst = bool(with_color), bool(with_inst)
        self.key = np.zeros(0, np.uint64); self.fix = np.zeros((0, 3), np.int64)
        self.bgr = np.zeros((0, 3), np.int64); self.id = np.zeros(0, np.int64)
        self.frame = np.zeros(0, np.int64)          # which frame (in order of arrival) a sample came from: for check_conditions only
        self.pw = np.zeros((0, 3))
        self.n_frames = 0
        self.status = 0

    def add_frames(self, cams, K, rows, cols, depth, bgr=None, inst=None):
        cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
        tot = dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0)
        if self.status:
            return dict(tot, status=self.status)
        for c in cams:
            pose(c)          # an invalid pose anywhere: nothing is added
        new = []
        for f, c in enumerate(cams):
            s = samples(c, K, rows, cols, np.asarray(depth)[f], self.p)
            for k_, v in s["counts"].items():
                tot[k_] += v
            n = len(s["row"])
            col = np.asarray(bgr)[f][s["row"], s["col"]].astype(np.int64) if self.with_color else np.zeros((n, 3), np.int64)
            ids = np.asarray(inst)[f][s["row"], s["col"]].astype(np.int64) if self.with_inst else np.full(n, -1, np.int64)
            new.append((pack(s["k"]), np.rint(s["pw"] * FIX).astype(np.int64), col, ids, np.full(n, self.n_frames + f, np.int64), s["pw"]))
        if len(self.key) + tot["n_sampled"] >= 1 << 31:
            raise ValueError("n_samples would reach 2^31")
        self.n_frames += len(cams)
        for name, i in (("key", 0), ("fix", 1), ("bgr", 2), ("id", 3), ("frame", 4), ("pw", 5)):
            setattr(self, name, np.concatenate([getattr(self, name)] + [x[i] for x in new]))
        if self.n_voxels() > self.p["max_voxels"] or self.n_pairs() > 2 * self.p["max_voxels"]:
            self.status = 3
        return dict(tot, status=self.status)

    def n_voxels(self):
        return len(np.unique(self.key))

    def n_pairs(self):
        lab = self.id >= 0
        return len(np.unique(np.stack([self.key[lab], self.id[lab].astype(np.uint64)], axis=-1), axis=0)) if lab.any() else 0

    def info(self):
        bad = self.status != 0
        return dict(n_samples=len(self.key), n_voxels=-1 if bad else self.n_voxels(), n_pairs=-1 if bad else self.n_pairs(),
                    status=self.status, with_color=int(self.with_color), with_inst=int(self.with_inst))

    def extract(self, cap=None):
        """step 7 -> dict(n_voxels, key (n, 3) int32, xyz (n, 3), count, bgr (n, 3) uint8, inst, votes); n = min(cap, n_voxels)"""
        if self.status:
            return dict(n_voxels=-1)
        keys, inv, count = np.unique(self.key, return_inverse=True, return_counts=True)          # ascending packed key
        V = len(keys)
        S = np.zeros((V, 3), np.int64); C = np.zeros((V, 3), np.int64)
        np.add.at(S, inv, self.fix)
        np.add.at(C, inv, self.bgr)
        xyz = S.astype(np.float64) / FIX / count.astype(np.float64)[:, None]
        bgr = ((2 * C + count[:, None]) // (2 * count[:, None])).astype(np.uint8)
        label = np.full(V, -1, np.int32); votes = np.zeros(V, np.int32)
        lab = self.id >= 0
        if lab.any():
            pairs, n = np.unique(np.stack([inv[lab], self.id[lab]], axis=-1), axis=0, return_counts=True)
            # most votes first, then the lowest id; the first row of a voxel wins
            order = np.lexsort((pairs[:, 1], -n, pairs[:, 0]))
            pv, first = np.unique(pairs[order, 0], return_index=True)
            label[pv] = pairs[order][first, 1]; votes[pv] = n[order][first]
        m = V if cap is None else min(int(cap), V)
        return dict(n_voxels=V, key=unpack(keys).astype(np.int32)[:m], xyz=xyz[:m], count=count.astype(np.int32)[:m], bgr=bgr[:m],
                    inst=label[:m], votes=votes[:m])

    def margins(self):
        """the smallest distance of a used sample's p_w / leaf to an integer and of p_w 2^30 to a half-integer"""
        if not len(self.pw):
            return dict(key=np.inf, fix=np.inf)
        q = self.pw / self.p["leaf"]
        x = self.pw * FIX
        return dict(key=float(np.abs(q - np.rint(q)).min()), fix=float(np.abs(x - np.floor(x) - 0.5).min()))
