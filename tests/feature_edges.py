"""Edge cases of the feature kernels (ORB, Hamming / L2 kNN-2, RANSAC): one table of named inputs
with the property each exists for.

test_feature_edges_cpu.py runs every case through the CPU oracle alone and checks that it shows
its property (so that a GPU comparison on the same table cannot pass on an empty result) and that
no pyramid level holds more candidates than the product's candidate buffer (above that the
product drops candidates in atomic order and has no defined answer);
test_gpu_feature_edges.py runs the same table on the GPU.

ORB cases: dict(name, image (a builder), nfeatures, nlevels, scale_factor, threshold, prop (a
sentence), and the keys check_orb_property reads).  The oracle's result dict is what the property
is checked on.
"""
import numpy as np

EDGE = 31                   # mcs_orb_core.h kOrbEdge
SEL_MAX = 4096              # mcs_fparams.h kOrbSelMax: more candidates on a level -> host ranking


# ---- image builders ------------------------------------------------------------------------------

def lattice(K, pitch=8, cols=72, val=255, rows=None):
    """Black image with K isolated single-pixel dots on a pitch-px lattice starting at (34, 34),
    row-major, `cols` dots to a row, and a 31-px margin after the last dot (so every dot is a
    level-0 keypoint and nothing else is: a dot's FAST circle is all black, a black pixel's circle
    holds at most one dot).  val: one gray level, or a function of the dot's index k."""
    rows = rows or (K + cols - 1) // cols
    h, w = 34 + pitch * (rows - 1) + 1 + EDGE, 34 + pitch * (cols - 1) + 1 + EDGE
    img = np.zeros((h, w), np.uint8)
    k = np.arange(K)
    v = np.array([val(int(i)) for i in k], np.uint8) if callable(val) else np.uint8(val)
    img[34 + pitch * (k // cols), 34 + pitch * (k % cols)] = v
    return img


def lattice_xy(K, pitch=8, cols=72):
    """(x, y) of the lattice's dots in row-major -- (y, x) ranking -- order."""
    k = np.arange(K)
    return np.stack([34 + pitch * (k % cols), 34 + pitch * (k // cols)], axis=1).astype(np.float32)


def ramp_val(k):
    """156 distinct gray levels 100..255 (37 and 156 are coprime)."""
    return 100 + (37 * k) % 156


def dot63():
    img = np.zeros((63, 63), np.uint8)
    img[31, 31] = 255
    return img


BORDER_DOTS = [(30, 36), (31, 44), (68, 52), (69, 60), (40, 30), (48, 31), (56, 64), (64, 65)]
BORDER_KEPT = [(48, 31), (31, 44), (68, 52), (56, 64)]      # (x, y): one response, so (y, x) order


def border():
    """100 x 96: dots one pixel inside and one pixel outside the 31-px edge on all four sides
    (x = 30 | 31, x = 68 | 69 of 100; y = 30 | 31, y = 64 | 65 of 96)."""
    img = np.zeros((96, 100), np.uint8)
    for x, y in BORDER_DOTS:
        img[y, x] = 255
    return img


def tiled():
    """A random 16 x 16 block tiled to 192 x 256 (w x h): the same corners 12 x 16 times over, so
    a handful of distinct responses shared by a thousand keypoints."""
    b = np.random.default_rng(11).integers(0, 256, (16, 16), dtype=np.uint8)
    return np.tile(b, (16, 12))


def noise(h, w, seed=None):
    return np.random.default_rng(h * 1000 + w if seed is None else seed).integers(
        0, 256, (h, w), dtype=np.uint8)


def mixed(h, w, seed=5):
    """Pixel noise on the left half, 6-px blocks of noise on the right: the fine levels find their
    corners in the first, the coarse levels (where pixel noise has averaged out) in the second, so
    every one of 12 levels at 1.2 has more candidates than a small nfeatures gives it quota."""
    rng = np.random.default_rng(seed)
    img = rng.integers(0, 256, (h, w), dtype=np.uint8)
    b = np.kron(rng.integers(0, 256, (h // 6 + 1, w // 6 + 1)), np.ones((6, 6)))[:h, :w]
    img[:, w // 2:] = b[:, w // 2:].astype(np.uint8)
    return img


def flat():
    return np.full((120, 160), 77, np.uint8)


# ---- the ORB table -------------------------------------------------------------------------------

def _orb(name, image, prop, nfeatures=500, nlevels=8, scale_factor=1.2, threshold=20, **kw):
    d = dict(name=name, image=image, prop=prop, nfeatures=nfeatures, nlevels=nlevels,
             scale_factor=scale_factor, threshold=threshold)
    d.update(kw)
    return d


LATTICE_K = (1, 64, 65, 128, 129, 4096, 4097)
ORB_CASES = [
    _orb(f"lattice_{K}", (lambda K=K: lattice(K)), f"exactly {K} level-0 keypoints, one response: "
         "the ranking is (y, x) alone; 64|65, 128|129: the sort network's padded size steps, "
         "4096|4097: device | host ranking", nfeatures=5000, nlevels=1, count=K, lattice=K,
         distinct=1)
    for K in LATTICE_K
] + [
    _orb("lattice_ramp_300", lambda: lattice(300, val=ramp_val), "156 distinct responses over 300 "
         "keypoints: ranking by response, then (y, x)", nfeatures=5000, nlevels=1, count=300,
         distinct=156),
    _orb("lattice_ramp_4096", lambda: lattice(4096, val=ramp_val), "the full 4096-entry network "
         "with 156 response groups", nfeatures=5000, nlevels=1, count=4096, distinct=156),
    _orb("lattice_cut_129", lambda: lattice(129), "nfeatures = 100 cuts inside the tie group: the "
         "last kept keypoint is (250, 42)", nfeatures=100, nlevels=1, count=100, distinct=1,
         last_xy=(250, 42)),
    _orb("dot63", dot63, "the smallest level with an eligible pixel: one keypoint at (31, 31), "
         "zero moments -> orientation (1, 0)", nlevels=1, count=1, last_xy=(31, 31), cs_sn=(1, 0)),
    _orb("border", border, "the edge rule on all four sides: dots at 31 and w - 32 survive, at 30 "
         "and w - 31 do not", nlevels=1, count=4, kept=BORDER_KEPT),
    _orb("tiled", tiled, "1,091 level-0 keypoints with 12 distinct responses: ties inside every "
         "response group", nfeatures=2000, nlevels=2, level0=1091, distinct0=12, min_levels=2),
] + [
    _orb(f"noise_{h}x{w}", (lambda h=h, w=w, kw=kw: noise(h, w, kw.get("seed"))), prop, nlevels=nl,
         **kw)
    for (h, w, nl, prop, kw) in [
        (8, 8, 12, "levels of 8 .. 1 px (the clamped reflection), no eligible pixel", dict(count=0)),
        (36, 40, 12, "levels of 40 x 36 .. 5 x 5 px, no eligible pixel", dict(count=0)),
        (62, 62, 8, "one pixel short of an eligible pixel", dict(count=0)),
        (64, 64, 8, "2 x 2 eligible pixels (one of them a keypoint), one tile, every row "
         "reflected", dict(count=1, seed=3)),
        (67, 65, 8, "width 65 = 1 mod 4, a second tile column of one pixel and a second tile row "
         "of three", dict(count=3, seed=14)),
        (72, 72, 8, "9 x 9 eligible pixels", dict(min_count=1)),
        (199, 131, 8, "one pixel short of an interior tile; widths 131, 109, 91 = 3, 1, 3 mod 4",
         dict(min_count=100, min_levels=3)),
        (132, 132, 3, "the smallest level with an interior tile", dict(min_count=100,
                                                                       min_levels=3)),
    ]
] + [
    _orb(f"scale_{s}" + ("" if nl == 4 else f"_l{nl}"), lambda: noise(264, 200), prop, nlevels=nl,
         scale_factor=s, min_count=100, min_levels=2, chain=chain)
    for (s, nl, chain, prop) in [
        (1.05, 4, False, "a fine pyramid through the one-launch kernel"),
        (1.5, 4, False, "a coarse pyramid through the one-launch kernel (levels 200, 133, 89, 59 "
         "wide)"),
        (1.99, 3, False, "the widest steps the one-launch kernel takes (200 -> 101 -> 51)"),
        (1.99, 4, True, "the per-level resize chain with bilinear steps either side of 2x "
         "(51 -> 25, 67 -> 33: the fourth level's step is past 2x)"),
        (2.0, 4, True, "the per-level resize chain, every step OpenCV's exact-2x area average"),
        (3.0, 4, True, "the per-level resize chain, bilinear steps of 3x"),
    ]
] + [
    _orb(f"threshold_{t}", lambda: noise(320, 240), prop, nlevels=4, threshold=t, **kw)
    for (t, prop, kw) in [
        (0, "every strict arc is a corner", dict(min_count=400)),
        (1, "threshold 1", dict(min_count=400)),
        (254, "only a 255 ring around a 0 (or the reverse) passes", dict()),
        (255, "no score exceeds 255: no keypoint", dict(count=0)),
    ]
] + [
    # (600 x 800 of `mixed`: every level has more candidates than its quota, so the keypoints
    # returned are the quotas' sum -- OpenCV's uncapped roundings gave nfeatures + 1 here)
    _orb(f"nfeatures_{nf}_l{nl}_s{s}", lambda: mixed(800, 600), prop, nfeatures=nf, nlevels=nl,
         scale_factor=s, count=nf, full=True, **kw)
    for (nf, nl, s, prop, kw) in [
        (0, 8, 1.2, "no keypoint asked for", {}),
        (1, 8, 1.2, "one keypoint: every quota but the last level's rounds to 0", {}),
        (7, 8, 1.2, "OpenCV's roundings sum to 8", dict(opencv_sum=8)),
        (14, 11, 1.2, "OpenCV's roundings sum to 15", dict(opencv_sum=15)),
        (24, 12, 1.2, "OpenCV's roundings sum to 25, and 24 x 32 B is a whole number of 256-B "
         "units: a 25th descriptor landed in the orientation table", dict(opencv_sum=25)),
    ]
] + [
    # (OpenCV's roundings sum to 90 here, but levels 6 .. 11 are under 63 px at any frame size the
    # suite may use, so only 82 of the 88 can exist: the case pins the quotas of the levels that do)
    _orb("nfeatures_88_l12_s1.5", lambda: mixed(800, 600), "12 levels at 1.5: six of them too "
         "small for a keypoint, the other six fill their quotas 30 20 13 9 6 4", nfeatures=88,
         nlevels=12, scale_factor=1.5, count=82, opencv_sum=90),
] + [
    _orb("flat", flat, "no corner anywhere", count=0),
]
ORB_BY_NAME = {c["name"]: c for c in ORB_CASES}
NFEATURES_CASES = [c["name"] for c in ORB_CASES if c["name"].startswith("nfeatures_")]


def orb_kwargs(case):
    return dict(nfeatures=case["nfeatures"], nlevels=case["nlevels"],
                scale_factor=case["scale_factor"])


def level_sizes(w, h, nlevels, scale_factor):
    """ORB's level sizes [(w_l, h_l)], OpenCV's float arithmetic (mcs_features.cpp orb_geom)."""
    out = []
    for l in range(nlevels):
        s = np.float32(np.float64(np.float32(scale_factor)) ** l)
        out.append((int(np.rint(np.float32(w) / s)), int(np.rint(np.float32(h) / s))))
    return out


def opencv_quotas(nfeatures, nlevels, scale_factor):
    """OpenCV's per-level split of nfeatures, uncapped (float arithmetic as ORB_Impl)."""
    f = np.float32(1.0 / np.float64(np.float32(scale_factor)))
    per = np.float32(nfeatures) * (np.float32(1) - f) / (
        np.float32(1) - np.float32(np.float64(f) ** nlevels))
    q = []
    for _ in range(nlevels - 1):
        q.append(int(np.rint(np.float32(per))))
        per = np.float32(per * f)
    return q + [max(nfeatures - sum(q), 0)]


_CAND = {}


def case_candidates(case):
    """Candidates per level of the case's image (the oracle asked for 10^6 keypoints: no quota
    binds), computed once."""
    from oracle import oracle
    if case["name"] not in _CAND:
        big = oracle.orb_detect(case["image"](), nfeatures=10 ** 6, nlevels=case["nlevels"],
                                scale_factor=case["scale_factor"], threshold=case["threshold"])
        _CAND[case["name"]] = np.bincount(big["level"], minlength=case["nlevels"]).tolist()
    return _CAND[case["name"]]


def candidate_caps(w, h, nlevels, scale_factor):
    """The product's candidate capacity per level: max(4096, w_l h_l / 8) (orb_geom)."""
    return [max(4096, (lw * lh) // 8) for lw, lh in level_sizes(w, h, nlevels, scale_factor)]


def check_orb_property(case, res):
    """The case shows what it is in the table for, on the oracle's result alone."""
    name = case["name"]
    n = len(res["xy"])
    assert n <= case["nfeatures"], (name, n)
    if "count" in case:
        assert n == case["count"], (name, n)
    if "min_count" in case:
        assert n >= case["min_count"], (name, n)
    if "min_levels" in case:
        assert len(np.unique(res["level"])) >= case["min_levels"], (name, np.unique(res["level"]))
    if "distinct" in case:
        assert len(np.unique(res["response"])) == case["distinct"], name
        assert (res["level"] == 0).all(), name
    if "lattice" in case:
        assert np.array_equal(res["xy"], lattice_xy(case["lattice"])), name
    if "last_xy" in case:
        assert tuple(res["xy"][-1]) == case["last_xy"], (name, res["xy"][-1])
    if "cs_sn" in case:
        assert tuple(res["cs_sn"][0]) == case["cs_sn"], (name, res["cs_sn"][0])
    if "kept" in case:
        assert [tuple(p) for p in res["xy"]] == case["kept"], (name, res["xy"])
    if "level0" in case:
        l0 = res["level"] == 0
        assert int(l0.sum()) == case["level0"], (name, int(l0.sum()))
        assert len(np.unique(res["response"][l0])) == case["distinct0"], name
    if "opencv_sum" in case:
        q = opencv_quotas(case["nfeatures"], case["nlevels"], case["scale_factor"])
        assert sum(q) == case["opencv_sum"] > case["nfeatures"], (name, q)
        if case.get("full"):
            # every level offers more candidates than OpenCV's quota: uncapped, the frame yields
            # more keypoints than nfeatures
            assert all(c >= k for c, k in zip(case_candidates(case), q)), name
    if "chain" in case:
        # a level step of 2x or more: the one-launch pyramid declines, the resize chain runs
        sizes = level_sizes(200, 264, case["nlevels"], case["scale_factor"])
        step2 = any(2 * a[0] <= b[0] or 2 * a[1] <= b[1] for a, b in zip(sizes[1:], sizes))
        assert step2 == case["chain"], (name, sizes)
    if name == "scale_2.0":
        assert level_sizes(200, 264, 4, 2.0) == [(200, 264), (100, 132), (50, 66), (25, 33)]


# ---- matcher and RANSAC cases --------------------------------------------------------------------

def hamming_complement():
    """t = [d, d], q = [~d]: distance 256 (bit 31 of the key distance << 23 | index) twice, the
    tie broken by index."""
    d = np.random.default_rng(3).integers(0, 256, (1, 32), dtype=np.uint8)
    return ~d, np.concatenate([d, d]), np.array([[0, 1]]), np.array([[256, 256]])


def hamming_far_indices(nq):
    """nq queries against 70,000 train descriptors whose nearest two lie past index 65,535 (index
    bits 16 and up of the key): (q, t, idx, dist)."""
    rng = np.random.default_rng(100 + nq)
    nt = 70000
    t = rng.integers(0, 256, (nt, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (nq, 32), dtype=np.uint8)
    first = 65536 + 7 * np.arange(nq)            # the nearest: the query with one bit flipped
    second = 69999 - 11 * np.arange(nq)          # the second: three bits flipped
    t[first] = q
    t[first, 0] ^= 1
    t[second] = q
    t[second, 5] ^= 7
    return (q, t, np.stack([first, second], axis=1),
            np.stack([np.full(nq, 1), np.full(nq, 3)], axis=1))


def hamming_straddle():
    """Exact duplicates of the query at train indices 65,535 and 65,536, and of a second query at
    65,536 + 1 and 69,000: equal distances rank by index across bit 16."""
    rng = np.random.default_rng(17)
    t = rng.integers(0, 256, (70000, 32), dtype=np.uint8)
    q = rng.integers(0, 256, (2, 32), dtype=np.uint8)
    t[65535] = t[65536] = q[0]
    t[69000] = t[65537] = q[1]
    return q, t, np.array([[65535, 65536], [65537, 69000]]), np.zeros((2, 2), np.int64)


def l2_extremes(dim):
    """t = q = [0 .. 0, 255 .. 255]: second distance 255 sqrt(dim), the largest an 8-bit descriptor
    pair has."""
    t = np.stack([np.zeros(dim), np.full(dim, 255.0)]).astype(np.float32)
    return t.copy(), t, np.array([[0, 1], [1, 0]]), np.float32(255.0 * np.sqrt(np.float64(dim)))


def l2_float_case(dim, nt, seed=0):
    """Float-path descriptors: integer-valued queries, a train set with negative values and one
    non-integer value (which alone takes the whole call off the exact path)."""
    rng = np.random.default_rng(seed * 7919 + dim * 31 + nt)
    t = rng.integers(-40, 60, (nt, dim)).astype(np.float32)
    t[nt // 2, dim // 2] += np.float32(0.5)
    nq = 9
    q = (t[rng.integers(0, nt, nq)] + rng.integers(-3, 4, (nq, dim))).astype(np.float32)
    return q, t


def _grid_points(n, rng):
    return rng.uniform(20, 600, (n, 2)).astype(np.float32)


_H_TRUE = np.array([[1.02, 0.03, 12.0], [-0.02, 0.98, -7.0], [2e-5, -1e-5, 1.0]])


def _apply(H, p):
    q = np.c_[p.astype(np.float64), np.ones(len(p))] @ H.T
    return (q[:, :2] / q[:, 2:]).astype(np.float32)


def ransac_case(name):
    """(src, dst, iters, seed, has_model) of the named RANSAC case."""
    rng = np.random.default_rng(23)
    if name == "collinear40":       # every triple collinear: every subset is rejected
        x = np.linspace(10, 400, 40).astype(np.float32)
        src = np.stack([x, 2 * x + 5], axis=1).astype(np.float32)
        return src, src + np.float32([3, 4]), 200, 0, False
    if name == "duplicates30":      # 30 copies of one correspondence: zero cross products
        src = np.tile(np.float32([[100, 50]]), (30, 1))
        return src, src + np.float32([2, 1]), 200, 0, False
    if name == "exact4_iters65":    # the fewest points the entry point scores
        src = np.float32([[10, 10], [500, 20], [480, 400], [30, 380]])
        return src, _apply(_H_TRUE, src), 65, 0, True
    if name == "exact5_iters1":     # one hypothesis
        src = np.float32([[10, 10], [500, 20], [480, 400], [30, 380], [250, 200]])
        return src, _apply(_H_TRUE, src), 1, 0, True
    if name.startswith("iters"):    # hypothesis counts around the wave and block sizes
        src = _grid_points(60, rng)
        dst = _apply(_H_TRUE, src) + rng.normal(0, 1.5, (60, 2)).astype(np.float32)
        dst[::5] += rng.uniform(-40, 40, dst[::5].shape).astype(np.float32)
        return src, dst, int(name[5:]), 1, None
    if name.startswith("n"):        # point counts around the scoring block's 256 threads
        n = int(name[1:])
        src = _grid_points(n, rng)
        dst = _apply(_H_TRUE, src)
        if n >= 8:      # (noise: the hypotheses' scores differ, the best one is not the first)
            dst += rng.normal(0, 1.5, (n, 2)).astype(np.float32)
            dst[::7] += rng.uniform(-40, 40, dst[::7].shape).astype(np.float32)
        return src, dst, 300, 2, None
    raise KeyError(name)


RANSAC_DEGENERATE = ("collinear40", "duplicates30", "exact4_iters65", "exact5_iters1")
RANSAC_SIZES = tuple(f"iters{i}" for i in (1, 63, 64, 65, 257)) + \
    tuple(f"n{n}" for n in (4, 5, 255, 256, 257))


# ---- the rig job at small counts -----------------------------------------------------------------

def lattice_rig(dots=(0, 1, 2, 5, 40)):
    """One-channel frames of the lattice's size holding that many dots of its first row."""
    shape = lattice(max(dots), rows=1).shape
    return [lattice(k, rows=1) if k else np.zeros(shape, np.uint8) for k in dots]


# (w, h, seed of rig.estimation_rig, nfeatures), 3 cameras, 3 levels.  What the pairs come to on
# the oracle (matches; RANSAC): 160 x 120 / 7: 0, 0.  160 x 120 / 60: 11 matches with a model of 10
# inliers that 25 hypotheses share, and 5 matches with every hypothesis rejected.  320 x 240 / 7:
# 2, 0.  320 x 240 / 60: 6 matches all rejected, and 4 (refused: more than 4 are needed).  The last
# two: 9 matches whose best score is the least a model needs, 4, shared by 160 (189) hypotheses,
# 14 (6) of them in the wave of the first, with 8 (6) different inlier masks among those -- only
# the first of the maximum gives the reference's homography.
RIG_SMALL = [(160, 120, 2, 7), (160, 120, 2, 60), (320, 240, 2, 7), (320, 240, 2, 60),
             (320, 240, 4, 200), (320, 240, 7, 100)]
RIG_TIED = [(320, 240, 4, 200), (320, 240, 7, 100)]
# The rig job's per-level resize chain (3 levels at 2.0: no one-launch pyramid, so no graph either;
# the resize runs with a frame stride over the cameras): (w, h, seed, nfeatures) of the smallest
# 4:3 rig -- widths in steps of 16, seeds 0 .. 7 -- on which the oracle gives every camera keypoints
# on two levels (level 1 is 96 x 72: 10 eligible rows) and every pair more than 4 matches; the
# oracle's keypoints per camera and matches per pair.
RIG_CHAIN = (192, 144, 4, 100)
RIG_CHAIN_KEYPOINTS = [21, 29, 38]
RIG_CHAIN_MATCHES = [5, 5]


def opencv_gray(bgr):
    b = np.asarray(bgr).astype(np.int32)
    return ((b[..., 0] * 1868 + b[..., 1] * 9617 + b[..., 2] * 4899 + 8192) >> 14).astype(np.uint8)


def oracle_pairs(frames, nfeatures, nlevels, ratio=0.75, scale_factor=1.2, levels=None):
    """The rig's estimation on the oracle as far as the matches: (keypoints per camera, per pair
    (src, dst) float32 arrays of the ratio-tested matches, query camera k + 1 against train k).
    levels: a list that receives the number of levels each camera has keypoints on."""
    from oracle import oracle
    feats = [oracle.orb_detect(f if f.ndim == 2 else opencv_gray(f), nfeatures=nfeatures,
                               nlevels=nlevels, scale_factor=scale_factor) for f in frames]
    if levels is not None:
        levels[:] = [len(np.unique(f["level"])) for f in feats]
    pairs = []
    for k in range(len(frames) - 1):
        a, b = feats[k + 1], feats[k]
        src = dst = np.zeros((0, 2), np.float32)
        if len(a["xy"]) and len(b["xy"]):
            idx, dist = oracle.hamming_knn2(a["desc"], b["desc"])
            q = np.nonzero((idx[:, 1] >= 0) & (dist[:, 0].astype(np.float64) <
                                               dist[:, 1].astype(np.float64) * ratio))[0]
            src, dst = a["xy"][q], b["xy"][idx[q, 0]]
        pairs.append((src, dst))
    return [len(f["xy"]) for f in feats], pairs
