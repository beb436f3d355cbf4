"""A numpy model of the fp32 accumulators of pairsnp_mfma_kernel (csrc/pairsnp_mfma.hip), for tests/test_fp32_range_model.py.

One matrix instruction adds the products of 64 sites to an fp32 accumulator register: an integer increment of magnitude <= 64, one
fp32 rounding.  The model forms, for a pair of samples, the increments in the kernel's unit order and adds them one at a time in
float32 (np.add.accumulate with dtype float32 is sequential), starting from zero at every range boundary -- a workgroup's range --;
the ranges' results are converted to integers and added exactly, as the kernel's integer atomics do.

Which sites an instruction takes (site s = 128 g + 32 w + b: group g, 32-site word w, bit b -- pack_kernel):
    consensus  step st = 0, 1 of group g takes the words st and 2 + st; units v -> accV, then x, y, z -> accS
               (v = "is a base", x = (-1)^X, y = (-1)^Y, z = x y, 0 where the site is no base; A=00 C=01 G=10 T=11 in Y X);
    general    a stage = 2 groups = 256 sites; unit (plane p, residue q) takes the stage's sites with s mod 4 = q;
               planes A, C, G, T x q = 0..3 -> accS, then N (= A & C & G & T) x q = 0..3 -> accV;
    count      256 sites (a pair of groups) at a time, residue q = 0..3 of the one N plane -> accV.
What the kernel and the host make of the sums:
    consensus  d = sum over ranges (3 V - S) >> 2,  nn = sum V;
    general    d = sum over ranges (L_range - S + 3 V) + the partial-code terms (exact integers, general_sparse.hip),  nn = L - c_i - c_j + sum V;
    count      nn = sites - c_i - c_j + sum V  (d is not the counting pass's: nothing to model)."""
import numpy as np

from exact_range_cases import MASK_OF, SITES_PER_GROUP, pairs


def f32_ranges(inc, per_group, bounds):
    """inc: integer increments of one accumulator in issue order, `per_group` of them per group of sites; bounds: the groups at which
    ranges begin and end ([0, .., groups]).  -> the accumulator's value at the end of every range, as Python ints."""
    out = []
    for g0, g1 in zip(bounds[:-1], bounds[1:]):
        # (the last range ends with the stream: its last stage may hang over the alignment by zero groups)
        a, b = int(g0 * per_group), (inc.size if g1 == bounds[-1] else int(g1 * per_group))
        out.append(int(np.add.accumulate(inc[a:b].astype(np.float32), dtype=np.float32)[-1]) if b > a else 0)
    return out


def range_bounds(groups, groups_per_range):
    """[0, r, 2 r, .., groups]: ranges of `groups_per_range` groups, the last one shorter"""
    return list(range(0, groups, int(groups_per_range))) + [groups]


def _pad(a, multiple):
    r = (-a.size) % multiple
    return a if r == 0 else np.concatenate([a, np.zeros(r, a.dtype)])


def _steps64(a):
    """per (group, step): the sum over the words st and 2 + st -> int32 [groups, 2]"""
    return _pad(a, SITES_PER_GROUP).reshape(-1, 2, 2, 32).sum(axis=(1, 3), dtype=np.int32)


def _residues(a):
    """per (256-site stage, residue class): the sum over the sites with s mod 4 = q -> int32 [stages, 4]"""
    return _pad(a, 2 * SITES_PER_GROUP).reshape(-1, 64, 4).sum(axis=1, dtype=np.int32)


class ConsensusModel:
    def __init__(self, seqs):
        m = MASK_OF[seqs]
        self.n, self.L = seqs.shape
        assert np.isin(m, (1, 2, 4, 8, 15)).all(), "consensus form: A, C, G, T or N only"
        self.v = (m != 15).astype(np.int8)
        self.x = np.where((m == 2) | (m == 8), -1, 1).astype(np.int8) * self.v
        self.y = np.where((m == 4) | (m == 8), -1, 1).astype(np.int8) * self.v
        self.z = self.x * self.y
        self._inc = {}

    def increments(self, i, j):
        """(accS stream, 6 per group: x, y, z of step 0, then of step 1; accV stream, 2 per group) -- formed once per pair"""
        if (i, j) not in self._inc:
            s = np.stack([_steps64(t[i] * t[j]) for t in (self.x, self.y, self.z)], axis=-1)
            self._inc[i, j] = (s.reshape(-1), _steps64(self.v[i] * self.v[j]).reshape(-1))
        return self._inc[i, j]

    def pair(self, i, j, bounds):
        incS, incV = self.increments(i, j)
        S, V = f32_ranges(incS, 6, bounds), f32_ranges(incV, 2, bounds)
        return sum((3 * v - s) >> 2 for s, v in zip(S, V)), sum(V)


class GeneralModel:
    def __init__(self, seqs, ref_d):
        m = MASK_OF[seqs]
        self.n, self.L = seqs.shape
        self.planes = [((m >> p) & 1).astype(np.uint8) for p in range(4)]
        self.isn = (m == 15).astype(np.uint8)
        self.c = self.isn.sum(axis=1, dtype=np.int64)
        self.ref_d = {(int(i), int(j)): int(d) for i, j, d in zip(*pairs(self.n), ref_d)}
        self._inc = {}

    def increments(self, i, j):
        """(accS stream, 16 per stage of two groups: planes A, C, G, T x residues 0..3; accV stream, 4 per stage: the N plane)"""
        if (i, j) not in self._inc:
            s = np.stack([_residues(p[i] & p[j]) for p in self.planes], axis=1)          # [stages, plane, q]
            self._inc[i, j] = (s.reshape(-1), _residues(self.isn[i] & self.isn[j]).reshape(-1))
        return self._inc[i, j]

    def pair(self, i, j, bounds):
        assert all(b % 2 == 0 for b in bounds[:-1]), "ranges of the general form begin at whole stages"
        incS, incV = self.increments(i, j)
        S, V = f32_ranges(incS, 8, bounds), f32_ranges(incV, 2, bounds)
        # the partial-code terms the fix-up adds: what the exact sums leave of the reference distance
        sparse = self.ref_d[i, j] - (self.L - int(incS.sum(dtype=np.int64)) + 3 * int(incV.sum(dtype=np.int64)))
        assert sparse >= 0
        d = sparse
        for g0, g1, s, v in zip(bounds[:-1], bounds[1:], S, V):
            d += min(self.L, g1 * SITES_PER_GROUP) - g0 * SITES_PER_GROUP - s + 3 * v
        return d, self.L - int(self.c[i]) - int(self.c[j]) + sum(V)


class CountModel:
    """in_place: the N plane of every site; else of the counted sites alone (those with two N samples or more -- no dense site, no list
    in these cases), re-packed in site order"""
    def __init__(self, seqs, in_place):
        isn = MASK_OF[seqs] == 15
        self.n, self.L = seqs.shape
        self.c = isn.sum(axis=1, dtype=np.int64)
        self.plane = (isn if in_place else isn[:, isn.sum(axis=0) >= 2]).astype(np.uint8)
        self.sites = self.plane.shape[1]
        self.groups = (self.sites + SITES_PER_GROUP - 1) // SITES_PER_GROUP
        self._inc = {}

    def increments(self, i, j):
        """accV stream, 4 per pair of groups"""
        if (i, j) not in self._inc:
            self._inc[i, j] = _residues(self.plane[i] & self.plane[j]).reshape(-1)
        return self._inc[i, j]

    def pair_nn(self, i, j, bounds):
        assert all(b % 2 == 0 for b in bounds[:-1]), "ranges of the counting form begin at whole pairs of groups"
        return self.L - int(self.c[i]) - int(self.c[j]) + sum(f32_ranges(self.increments(i, j), 2, bounds))
