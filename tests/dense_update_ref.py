"""The numpy statement of esl_dense_remove_frames / _move_frames / _purge / _slots_get (include/esl.h, "the dense map", steps 8-11) on
top of tests/dense_ref.py, whose DenseMap keeps one row per sample.  Removing a frame deletes one equal row (key, fixed-point terms,
colour, id) per used sample; a sample that finds no equal row is kept as a DEBT row, so that the per-voxel integer sums the device
holds (rows minus debts) can be audited by the rules of step 9.  The sets of voxel keys and of (key, id) pairs claimed since the last
purge stand for the tables' slots.  Test infrastructure only: nothing here is imported by the package."""
import numpy as np

import dense_ref as dr

ROW_FIELDS = ("key", "fix", "bgr", "id", "frame", "pw")
ZERO_COUNTS = dict(n_sampled=0, n_zero=0, n_depth_out=0, n_key_out=0, n_used=0)


def row_tuple(key, fix, bgr, i):
    return (int(key), int(fix[0]), int(fix[1]), int(fix[2]), int(bgr[0]), int(bgr[1]), int(bgr[2]), int(i))


class DenseUpdateMap(dr.DenseMap):
    """DenseMap plus remove_frames / move_frames / purge / slots, as the C calls"""

    def __init__(self, with_color=True, with_inst=True, **over):
        super().__init__(with_color, with_inst, **over)
        self.n_samples = 0
        self.claim_v = set()          # packed keys claimed since begin or the last purge
        self.claim_p = set()          # (packed key, id)
        self.debt = []                # row tuples that were removed without having been there

    # ---- the tables as the device holds them ----------------------------------------------------------------------------------------
    def tables(self):
        """per claimed voxel: count, S (3), colour sums (3); per claimed pair: count -- rows minus debts, as int64"""
        vk = sorted(self.claim_v)
        vi = {k: i for i, k in enumerate(vk)}
        cnt = np.zeros(len(vk), np.int64); S = np.zeros((len(vk), 3), np.int64); Cs = np.zeros((len(vk), 3), np.int64)
        pk = sorted(self.claim_p)
        pi = {k: i for i, k in enumerate(pk)}
        pc = np.zeros(len(pk), np.int64)
        idx = np.array([vi[int(k)] for k in self.key], np.int64)
        np.add.at(cnt, idx, 1); np.add.at(S, idx, self.fix); np.add.at(Cs, idx, self.bgr)
        for k, i in zip(self.key, self.id):
            if i >= 0:
                pc[pi[(int(k), int(i))]] += 1
        for t in self.debt:
            if t[0] not in vi:
                continue          # no voxel: the sample subtracted nothing
            j = vi[t[0]]
            cnt[j] -= 1; S[j] -= np.array(t[1:4]); Cs[j] -= np.array(t[4:7])
            if t[7] >= 0 and (t[0], t[7]) in pi:
                pc[pi[(t[0], t[7])]] -= 1
        return dict(vk=vk, cnt=cnt, S=S, C=Cs, pk=pk, pc=pc, vi=vi)

    def audit(self, n_missing=0):
        """step 9 -> (live voxels, dead voxels, live pairs, dead pairs, inconsistent)"""
        t = self.tables()
        cnt, pc = t["cnt"], t["pc"]
        dead = cnt == 0
        bad = n_missing > 0 or bool((cnt < 0).any()) or bool((dead & ((t["S"] != 0).any(-1) | (t["C"] != 0).any(-1))).any())
        bad = bad or bool((pc < 0).any())
        for (k, _), n in zip(t["pk"], pc):
            if n > 0 and cnt[t["vi"][k]] == 0:
                bad = True          # a live pair of a dead voxel
        return int((cnt > 0).sum()), int(dead.sum()), int((pc > 0).sum()), int((pc == 0).sum()), bad

    # ---- the calls ----------------------------------------------------------------------------------------------------------------------
    def add_frames(self, cams, K, rows, cols, depth, bgr=None, inst=None):
        n0 = len(self.key)
        res = super().add_frames(cams, K, rows, cols, depth, bgr, inst)
        if len(self.key) == n0 and res["n_sampled"] == 0:
            return res          # an invalid map: nothing was added
        self.n_samples += res["n_used"]
        for k, i in zip(self.key[n0:], self.id[n0:]):
            self.claim_v.add(int(k))
            if i >= 0:
                self.claim_p.add((int(k), int(i)))
        # step 11: capacity counts claimed slots
        self.status = 3 if len(self.claim_v) > self.p["max_voxels"] or len(self.claim_p) > 2 * self.p["max_voxels"] else 0
        return dict(res, status=self.status)

    def remove_frames(self, cams, K, rows, cols, depth, bgr=None, inst=None):
        cams = np.asarray(cams, dtype=np.float64).reshape(-1, 7)
        tot = dict(ZERO_COUNTS, n_missing=0, n_emptied=0)
        if self.status:
            return dict(tot, status=self.status)
        for c in cams:
            dr.pose(c)          # an invalid pose anywhere: nothing is removed
        where = {}
        for j in range(len(self.key)):
            where.setdefault(row_tuple(self.key[j], self.fix[j], self.bgr[j], self.id[j]), []).append(j)
        dead_before = self.audit()[1]
        gone = []
        for f, c in enumerate(cams):
            s = dr.samples(c, K, rows, cols, np.asarray(depth)[f], self.p)
            for k_, v in s["counts"].items():
                tot[k_] += v
            n = len(s["row"])
            key = dr.pack(s["k"]); fix = np.rint(s["pw"] * dr.FIX).astype(np.int64)
            col = np.asarray(bgr)[f][s["row"], s["col"]].astype(np.int64) if self.with_color else np.zeros((n, 3), np.int64)
            ids = np.asarray(inst)[f][s["row"], s["col"]].astype(np.int64) if self.with_inst else np.full(n, -1, np.int64)
            for j in range(n):
                t = row_tuple(key[j], fix[j], col[j], ids[j])
                if t[0] not in self.claim_v or (t[7] >= 0 and (t[0], t[7]) not in self.claim_p):
                    tot["n_missing"] += 1          # no voxel, or a voxel without this pair
                    self.debt.append(t)
                elif where.get(t):
                    gone.append(where[t].pop())
                else:
                    self.debt.append(t)          # the slots exist, the sums do not hold this sample
        keep = np.ones(len(self.key), bool); keep[gone] = False
        for name in ROW_FIELDS:
            setattr(self, name, getattr(self, name)[keep])
        self.n_samples -= tot["n_used"]
        _, dead, _, _, bad = self.audit(tot["n_missing"])
        tot["n_emptied"] = dead - dead_before
        if bad:
            self.status = 4
        else:
            assert not self.debt, "sums that cancel without their rows matching: not a case the statement covers"
        return dict(tot, status=self.status)

    def move_frames(self, cams_old, cams_new, K, rows, cols, depth, bgr=None, inst=None):
        old = np.asarray(cams_old, dtype=np.float64).reshape(-1, 7); new = np.asarray(cams_new, dtype=np.float64).reshape(-1, 7)
        assert old.shape == new.shape
        res = dict(removed=dict(ZERO_COUNTS, n_missing=0, n_emptied=0, status=self.status), added=dict(ZERO_COUNTS, status=self.status),
                   n_frames_moved=0, n_frames_same=0)
        if self.status or not len(old):
            return res
        for c in list(new) + list(old):
            dr.pose(c)
        mv = [f for f in range(len(old)) if old[f].tobytes() != new[f].tobytes()]
        per = len(range(0, rows, self.p["stride"])) * len(range(0, cols, self.p["stride"]))
        if self.n_samples + per * len(mv) >= 1 << 31:
            raise ValueError("n_samples would reach 2^31")
        res["n_frames_moved"], res["n_frames_same"] = len(mv), len(old) - len(mv)
        if not mv:
            return res

        def sub(a):
            return None if a is None else np.asarray(a)[mv]
        res["removed"] = self.remove_frames(old[mv], K, rows, cols, sub(depth), sub(bgr), sub(inst))
        res["added"]["status"] = self.status
        if not self.status:
            res["added"] = self.add_frames(new[mv], K, rows, cols, sub(depth), sub(bgr), sub(inst))
        return res

    def slots(self):
        if self.status:
            return dict(voxel_slots=-1, dead_voxels=-1, pair_slots=-1, dead_pairs=-1)
        lv, dv, lp, dp = self.audit()[:4]
        return dict(voxel_slots=lv + dv, dead_voxels=dv, pair_slots=lp + dp, dead_pairs=dp)

    def purge(self):
        before = self.slots()
        if not self.status:
            self.claim_v = {int(k) for k in self.key}
            self.claim_p = {(int(k), int(i)) for k, i in zip(self.key, self.id) if i >= 0}
        return before, self.slots()

    def info(self):
        return dict(super().info(), n_samples=self.n_samples)
