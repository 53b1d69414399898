"""The small scenes of tests/test_segment_cpu.py and tests/test_gpu_segment_edges.py: deterministic clouds of at most about 5 000
points, each built for one place where csrc/segment.hip can go wrong without the workload-sized scenes noticing (an odd k, rings
that stay empty, a grid one cell thick, a label that travels a whole chain, the segment tables' widths and caps).  A builder returns
(xyz float32 [n, 3], rgb uint32 [n], ind int32 [m] ascending, the option keywords it is meant to run with), some a fifth value that
says what was planted (the cluster, blob or run of every point); the rule scenes built by hand come with the outcome the rules give
them (rule_scenes()).  Coordinates of the tied scenes are small binary fractions, so every
d2 is exact in float32 in any evaluation order; the others are passed through untie(), so the literal twin's assertion that no two
candidates of a row tie holds outright."""
import numpy as np

KMAX = 128
P6 = 5                                      # a colour step the reference's point threshold (6: <= 36 joins) joins; two steps (100) it does not


def pack(r, g, b):
    return (np.asarray(r, np.uint32) << 16) | (np.asarray(g, np.uint32) << 8) | np.asarray(b, np.uint32)


def _f(a):
    return np.ascontiguousarray(np.asarray(a, np.float32).reshape(-1, 3))


def _all(n):
    return np.arange(n, dtype=np.int32)


def _untie(xyz, k):
    # (the twin's own helper: imported here, at the call, because tests/test_segment_cpu.py imports this module)
    from tests.test_segment_cpu import untie
    return untie(xyz, _all(len(xyz)), k)


PATCH_COLOURS = [(200, 40, 40), (40, 200, 40), (40, 40, 200), (200, 200, 40), (40, 200, 200), (200, 40, 200)]


def patch_scene(n, seed, salt=0.03, scale=1.0, close=False):
    """Six colour patches and a gradient patch (red 20..200 along x) on unit squares of a slightly wavy sheet at z ~ 1,
    colour noise of +-1 per channel, and `salt` of the points recoloured at random.  close: patches 1 and 2 get colours
    within the region threshold of patch 0's (the homogeneous merging joins them).  Returns xyz, rgb, patch id, salt mask."""
    rng = np.random.default_rng(seed)
    patch = rng.integers(0, 7, n)
    u, v = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    x, y = (patch % 4) + u, (patch // 4) + v
    z = 1.0 + 0.05 * np.sin(3 * x) * np.cos(2 * y) + rng.normal(0, 1e-3, n)
    cols = list(PATCH_COLOURS)
    if close:
        cols[1], cols[2] = (202, 42, 41), (198, 38, 42)
    base = np.array(cols + [(0, 90, 160)])[patch]
    base[patch == 6, 0] = np.round(20 + 180 * u[patch == 6])
    rgb = base + rng.integers(-1, 2, (n, 3))
    is_salt = rng.uniform(size=n) < salt
    rgb[is_salt] = rng.integers(0, 256, (int(is_salt.sum()), 3))
    xyz = (np.c_[x, y, z] * [scale, scale, 1.0]).astype(np.float32)
    return xyz, pack(*rgb.T), patch, is_salt


# ---------------------------------------------------------------- the subset k-NN: parities of k, ties, rings
def untied_sheet(m, seed=0):
    """m points of the patch scene with every pair of distances from one point untied (untie() over all m candidates), so the
    first m' points are tie-free for every k too."""
    xyz, rgb, _, _ = patch_scene(m, 100 + seed, salt=0.05)
    return _untie(xyz, m), rgb, _all(m), dict(min_cluster_size=5)


def lattice(nx, ny, nz):
    """The integer points of a box: every d2 is a small integer, most of them shared by many pairs.  The order of a list is
    (d2, index) and nothing else; the reference is brute_knn, not the twin, which refuses ties."""
    g = np.stack(np.meshgrid(np.arange(nx), np.arange(ny), np.arange(nz), indexing="ij"), -1).reshape(-1, 3)
    g = g[np.random.default_rng(7).permutation(len(g))]                       # (index order is not raster order)
    rgb = pack(40 + 20 * (g[:, 0] % 3), 90, 160)
    return _f(g), rgb, _all(len(g)), dict(min_cluster_size=1)


def far_clusters(k):
    """Three clusters of about 0.4 k points, 0.5 across, 60 and 90 apart along x (the box is flat, so the density grid has tens
    of cells between them), and two lone points between them: every point's k-th neighbour lies in another cluster, behind
    rings that are empty for many steps.  Returns the cluster of every point (-1: lone) as a fifth value."""
    rng = np.random.default_rng(1000 + k)
    per = max(2, int(round(0.4 * k)))
    centres = np.array([[0.0, 0.0, 0.0], [60.0, 5.0, 0.2], [150.0, -5.0, -0.1]])
    pts = [c + rng.uniform(-0.25, 0.25, (per, 3)) for c in centres] + [np.array([[27.0, 1.0, 0.1], [101.0, -2.0, 0.0]])]
    member = np.concatenate([np.full(per, j) for j in range(3)] + [[-1, -1]]).astype(np.int32)
    xyz = np.concatenate(pts)
    o = rng.permutation(len(xyz))
    xyz, member = _f(xyz[o]), member[o]
    col = np.array([(200, 40, 40), (40, 200, 40), (40, 40, 200), (120, 120, 120)])[member]
    kw = dict(region_neighbour_number=k, neighbour_number=min(30, k), min_cluster_size=2, distance_threshold=1000.0)
    return _untie(xyz, len(xyz)), pack(*col.T), _all(len(xyz)), kw, member


def line(m):
    """m points along x with unequal spacings, y = 0 and z = 1: the grid is one cell thick in y and in z.  Colour blocks of 500
    points, every other point of a block one step off.  Untied deep enough for a list of every third point."""
    rng = np.random.default_rng(5)
    x = np.cumsum(rng.uniform(0.5, 1.5, m)) * 0.01
    xyz = _f(np.c_[x, np.zeros(m), np.ones(m)])
    block = np.arange(m) // 500
    rgb = pack((37 * block) % 200 + (np.arange(m) % 2), (91 * block) % 200, 60)
    return _untie(xyz, min(m, 3 * (KMAX + 8))), rgb, _all(m), dict(min_cluster_size=100)


# ---------------------------------------------------------------- the growth: a label that travels a whole chain
def _colour_walk(m):
    """m colours, consecutive ones one step of P6 apart in one channel, no two that are two apart within the point threshold: a
    boustrophedon through the colour cube (a turn costs 2 P6^2 = 50, a straight pair of steps (2 P6)^2 = 100, both > 36)."""
    side = 255 // P6 + 1
    t = np.arange(m)
    a, b, c = t % side, (t // side) % side, t // (side * side)
    b = np.where(c % 2 == 1, side - 1 - b, b)
    a = np.where((t // side) % 2 == 1, side - 1 - a, a)
    assert c.max() < side
    return pack(P6 * a, P6 * b, P6 * c)


def snake(m, order):
    """A chain of m points along x.  The gaps shrink by one unit per step (whole numbers of 1 / 1024, exact in float32), so the
    nearest neighbour of every point is the next one: with neighbour_number 2 the growth graph is the directed path head ->
    tail, with 3 it also has the edges back.  Colours: _colour_walk.  One segment needs the head to hold cloud index 0 (no
    other point reaches the whole path); `order` says which cloud index the rest of the chain gets:
    "ascending"   0, 1, 2, ..: every hop goes to the next index;
    "descending"  0, m - 1, m - 2, .., 1: after the first, every hop goes to a SMALLER index, and index 1, the smallest after
                  the seed, sits at the far end, m - 1 hops against index order away;
    "shuffled"    0, then a fixed permutation.
    region_neighbour_number is 8: within 16 candidates no two sums of gaps are equal (the twin's assertion holds)."""
    assert m <= 4097
    gaps = 6000 - np.arange(m - 1)
    x = np.concatenate([[0], np.cumsum(gaps)])
    assert x[-1] < 2 ** 24
    chain = _f(np.c_[x / 1024.0, np.zeros(m), np.ones(m)])
    if order == "ascending":
        index = np.arange(m)
    elif order == "descending":
        index = np.concatenate([[0], np.arange(m - 1, 0, -1)])
    elif order == "shuffled":
        index = np.concatenate([[0], 1 + np.random.default_rng(12).permutation(m - 1)])
    else:
        raise ValueError(order)
    xyz, rgb = np.zeros((m, 3), np.float32), np.zeros(m, np.uint32)
    xyz[index], rgb[index] = chain, _colour_walk(m)
    return xyz, rgb, _all(m), dict(region_neighbour_number=8, min_cluster_size=1)


# ---------------------------------------------------------------- the segment tables: widths, the cap, the means
BLOB_SIZES = (1, 2, 3, 4, 5, 8, 9)


def blobs(S):
    """S blobs of 20 points, 0.4 across and 3 apart on a 3 x 3 raster, each of one colour, the colours further apart than every
    threshold: exactly S segments, regions and clusters.  With 30 neighbours searched every blob's lists reach into others."""
    rng = np.random.default_rng(200 + S)
    cols = [(20, 20, 20), (220, 30, 30), (30, 220, 30), (30, 30, 220), (220, 220, 30), (30, 220, 220), (220, 30, 220), (120, 120, 120),
            (240, 240, 240)]
    which = np.repeat(np.arange(S), 20)[rng.permutation(20 * S)]
    xyz = np.c_[3.0 * (which % 3), 3.0 * (which // 3), np.ones(len(which))] + rng.uniform(-0.2, 0.2, (len(which), 3))
    kw = dict(region_neighbour_number=30, neighbour_number=10, min_cluster_size=20)
    return _untie(_f(xyz), len(xyz)), pack(*np.array(cols)[which].T), _all(len(xyz)), kw, which


HUB_COLOUR = (100, 100, 100)


def hub(n_sat, keep):
    """The integer points of the disc x^2 + y^2 <= 25, one colour, in a fixed shuffled order, and then n_sat <= 12 single
    points of distinct colours, each 1/4, 1/2 or 3/4 outwards of another of the disc's 12 rim points (x^2 + y^2 = 25): the d2 of
    the hub segment to satellite j is 1/16 (2 of them), 1/4 (4) or 9/16 (6) exactly, whichever k >= 2 neighbours are searched,
    and the satellites' index order is not their distance order.  The satellites' colours lie beyond the point threshold (1) and
    within the region threshold (5) of the hub's: rule 8 merges exactly the satellites the hub's capped list keeps, so the
    clusters show which of two tied satellites the cap kept.  region_neighbour_number = keep is also the k of the search: with
    keep = 1 no list holds a neighbour, every point is a segment and no segment has a neighbour segment."""
    assert n_sat <= 12
    g = np.stack(np.meshgrid(np.arange(-5, 6), np.arange(-5, 6), indexing="ij"), -1).reshape(-1, 2)
    g = g[(g ** 2).sum(1) <= 25]
    g = g[np.lexsort((g[:, 1], g[:, 0], (g ** 2).sum(1)))]
    rim = g[(g ** 2).sum(1) == 25]
    # with 4 neighbours searched a point of the disc keeps three of its four unit neighbours, the smaller indices: in most index
    # orders some point is kept by nobody and the disc falls apart.  This order grows it whole from index 0 (the CPU test checks)
    tip = np.abs(g).max(1) == 5
    g = g[np.lexsort((g[:, 1], g[:, 0], (g ** 2).sum(1), ~tip))][np.random.default_rng(140).permutation(len(g))]
    out = np.where(np.abs(rim[:, :1]) >= np.abs(rim[:, 1:]), np.c_[np.sign(rim[:, 0]), np.zeros(len(rim))],
                   np.c_[np.zeros(len(rim)), np.sign(rim[:, 1])])
    step = np.array([0.75, 0.5, 0.75, 0.25, 0.75, 0.5, 0.5, 0.75, 0.25, 0.75, 0.5, 0.75])
    sat = (rim + out * step[:, None])[:n_sat]
    dc = [(2, 0, 0), (0, 2, 0), (0, 0, 2), (2, 2, 0), (0, 2, 2), (2, 0, 2), (2, 2, 2), (-2, 0, 0), (0, -2, 0), (0, 0, -2), (-2, -2, 0),
          (0, -2, -2)]
    col = np.concatenate([np.tile(HUB_COLOUR, (len(g), 1)), np.array(HUB_COLOUR) + np.array(dc[:n_sat])])
    xy = np.concatenate([g.astype(np.float64), sat])
    kw = dict(region_neighbour_number=keep, neighbour_number=keep, min_cluster_size=1, point_color_threshold=1.0)
    return _f(np.c_[xy, np.ones(len(xy))]), pack(*col.T), _all(len(xy)), kw, len(g)


def thirds():
    """Five runs of points on a line, one segment each at point threshold 2: A (3 points, red 200, 201, 201: the mean 200.67 is
    stored as 200), B (7 points, green sum 704: 100.57 stored as 100), then D (red 205), E (green 105) and F (red 196), 5 points
    each.  With the region threshold 5 (a difference < 25 merges) the truncated means merge A with F (16) and neither A with D nor
    B with E (25); rounded means would merge A with D and B with E and leave F alone.  Returns the run of every point too."""
    runs = [[(200, 50, 50), (201, 50, 50), (201, 50, 50)],
            [(90, g, 30) for g in (100, 101, 101, 101, 100, 101, 100)],
            [(205, 50, 50)] * 5, [(90, 105, 30)] * 5, [(196, 50, 50)] * 5]
    x0 = [10.0, 30.0, 11.5, 32.5, 8.5]                                           # D right of A, F left of A, E right of B
    rng = np.random.default_rng(3)
    xs, cols, run = [], [], []
    for j, (r, a) in enumerate(zip(runs, x0)):
        xs += list(a + np.cumsum(rng.uniform(0.1, 0.2, len(r))))
        cols += r
        run += [j] * len(r)
    xyz = _f(np.c_[xs, np.zeros(len(xs)), np.ones(len(xs))])
    kw = dict(region_neighbour_number=30, neighbour_number=30, min_cluster_size=1, point_color_threshold=2.0)
    return _untie(xyz, len(xyz)), pack(*np.array(cols).T), _all(len(xyz)), kw, np.array(run)


# ---------------------------------------------------------------- the rule scenes built by hand
def _line(xs, cols, order=None):
    xyz = np.c_[np.asarray(xs, np.float32), np.zeros(len(xs)), np.ones(len(xs))].astype(np.float32)
    rgb = pack(*np.asarray(cols).T)
    if order is not None:
        xyz, rgb = xyz[order], rgb[order]
    return xyz, rgb


def beyond_30(neighbour_number=30):
    """A point, 35 points of another colour, and a point of the first colour that is the 37th entry of the first one's list."""
    A, B = (10, 10, 10), (200, 10, 10)
    xs = [0.0] + [1.0 + 0.37 * j for j in range(35)] + [40.0]
    xyz, rgb = _line(xs, [A] + [B] * 35 + [A])
    return xyz, rgb, _all(len(xs)), dict(neighbour_number=neighbour_number)


def directed_pair(u_first):
    """u, v, w of one colour at 0, 1, 1.5 with 2 entries per list: u -> v, v -> w, w -> v.  In the order v, w, u no flood reaches u."""
    xyz, rgb = _line([0.0, 1.0, 1.5], [(50, 50, 50)] * 3, order=None if u_first else [1, 2, 0])
    return xyz, rgb, _all(3), dict(neighbour_number=2, region_neighbour_number=2)


POINT_THRESHOLD_PAIRS = (((6, 0, 0), 1), ((6, 1, 0), 2), ((4, 4, 2), 1), ((4, 4, 3), 2))    # 36 joins, 37 and 41 do not


def threshold_pair(colour):
    """Two points, black and `colour`, at the reference's point threshold 6."""
    xyz, rgb = _line([0.0, 1.0], [(0, 0, 0), colour])
    return xyz, rgb, _all(2), dict()


def region_threshold_cases():
    """(two segment colours, the d2 between them, the regions rule 8 leaves): a colour difference of exactly 25 does not merge,
    16 does; d2 == 100 is near enough, the next float is not."""
    above = float(np.nextafter(np.float32(100), np.float32(200)))
    return (([(10, 10, 10), (15, 10, 10)], 1.0, 2), ([(10, 10, 10), (14, 10, 10)], 1.0, 1), ([(10, 10, 10), (13, 14, 10)], 1.0, 2),
            ([(10, 10, 10), (14, 10, 10)], 100.0, 1), ([(10, 10, 10), (14, 10, 10)], above, 2))


def region_threshold_points(colours, d2):
    """region_threshold_cases as points: 3 points of the first colour and 2 of the second on a line, the nearest pair sqrt(d2)
    apart (1, 10, or the float after 10), grown apart at point threshold 1."""
    gap = {1.0: 1.0, 100.0: 10.0}.get(d2, float(np.nextafter(np.float32(10), np.float32(20))))
    xs = [-0.5, -0.25, 0.0, gap, gap + 0.25]
    xyz, rgb = _line(xs, [colours[0]] * 3 + [colours[1]] * 2)
    assert np.float32(xyz[3, 0] * xyz[3, 0]) == np.float32(d2) or d2 > 100.0 and np.float32(xyz[3, 0] * xyz[3, 0]) > 100.0
    return xyz, rgb, _all(5), dict(min_cluster_size=1, point_color_threshold=1.0)


COMPACTION_COLOURS = [(0, 0, 0), (100, 0, 0), (0, 100, 0), (0, 0, 100)]


def compaction_tables():
    """Rule 9 and 10 on tables: (option keywords, counts, colours, lists, segment of every point, (seg_region or None, clusters,
    point_cluster)).  Four segments in a row 0 - 1 - 2 - 3, sizes 5, 2, 6, 1, min 4: region 1 moves into its nearest (segment 2,
    d2 1 against 4), region 3 into region 2, the emptied regions are compacted away in place; an emptied FIRST region takes the
    last one's place, so the cluster order changes; a region with no list stays and is erased by the size limit, as is one
    above the maximum."""
    col = COMPACTION_COLOURS
    return ((dict(min_cluster_size=4), [5, 2, 6, 1], col, [[(1, 4.0)], [(0, 4.0), (2, 1.0)], [(1, 1.0), (3, 9.0)], [(2, 9.0)]],
             [0] * 5 + [1] * 2 + [2] * 6 + [3], ([0, 2, 2, 2], 2, [0] * 5 + [1] * 9)),
            (dict(min_cluster_size=4), [2, 6, 5], col[:3], [[(1, 1.0)], [(0, 1.0), (2, 4.0)], [(1, 4.0)]],
             [0] * 2 + [1] * 6 + [2] * 5, ([1, 1, 2], 2, [1] * 8 + [0] * 5)),
            (dict(min_cluster_size=4, max_cluster_size=5), [2, 6, 5], col[:3], [[], [(2, 4.0)], [(1, 4.0)]],
             [0] * 2 + [1] * 6 + [2] * 5, (None, 1, [-1] * 8 + [0] * 5)))


def compaction_points(case):
    """The compaction_tables cases as points: runs of one colour on a line.  Cases 0 and 1: 1 / 16 between the points of a run,
    the nearest pair of neighbouring runs sqrt(d2) apart; every run sees every other (the lists hold all points), which adds
    entries to the tables and changes no decision: the nearest region of a small one is still its neighbour in the row.  Case 2,
    the region with no list: 2 entries per list, a pair of points far from the rest, and two chains whose gaps shrink (every
    point's one neighbour is the next of its own run), so no list crosses a segment at all."""
    if case == 2:
        runs = [[0.0, 0.5], list(100 + np.cumsum([0, 5, 4.5, 4, 3.5, 3])), list(130 + np.cumsum([0, 4, 3.5, 3, 2.5]))]
        xyz, rgb = _line(sum(runs, []), sum(([COMPACTION_COLOURS[j]] * len(r) for j, r in enumerate(runs)), []))
        return xyz, rgb, _all(len(xyz)), dict(min_cluster_size=4, max_cluster_size=5, region_neighbour_number=2, neighbour_number=2)
    counts, gaps = (([5, 2, 6, 1], [2.0, 1.0, 3.0]), ([2, 6, 5], [1.0, 2.0]))[case]
    xs, cols, x = [], [], 0.0
    for j, n in enumerate(counts):
        xs += [x + i / 16.0 for i in range(n)]
        cols += [COMPACTION_COLOURS[j]] * n
        x = xs[-1] + (gaps[j] if j < len(gaps) else 0.0)
    xyz, rgb = _line(xs, cols)
    return xyz, rgb, _all(len(xs)), dict(min_cluster_size=4)


def rule_scenes():
    """(name, scene, expectation) for every rule scene that is a cloud: the expectation holds `segments` (count, segment of every
    point) for the growth and / or `clusters` (count, label of every point) and `regions` for the whole call."""
    out = [("beyond_30", beyond_30(), dict(segments=(3, [0] + [1] * 35 + [2]))),
           ("beyond_30_looks_at_40", beyond_30(40), dict(segments=(2, [0] + [1] * 35 + [0]))),
           ("directed_pair_u_first", directed_pair(True), dict(segments=(1, [0, 0, 0]))),
           ("directed_pair_u_last", directed_pair(False), dict(segments=(2, [0, 0, 1])))]
    for c, want in POINT_THRESHOLD_PAIRS:
        out.append(("point_threshold_%d_%d_%d" % c, threshold_pair(c), dict(segments=(want, [0, want - 1]))))
    for j, (colours, d2, regions) in enumerate(region_threshold_cases()):
        pc = [0] * 5 if regions == 1 else [0, 0, 0, 1, 1]
        out.append(("region_threshold_%d" % j, region_threshold_points(colours, d2), dict(segments=(2, [0, 0, 0, 1, 1]), regions=regions,
                                                                                             clusters=(regions, pc))))
    tabs = compaction_tables()
    for case in (0, 1, 2):
        counts, seg, (_, nc, pc) = tabs[case][1], tabs[case][4], tabs[case][5]
        out.append(("compaction_%d" % case, compaction_points(case), dict(segments=(len(counts), seg), regions=len(counts), clusters=(nc, pc))))
    return out
