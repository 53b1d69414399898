"""The mesh finishing (csrc/mesh.h, include/sfmhip.h rules M1-M7) on the CPU, through a g++ build of the header
the device kernels compile (tests/stub/mesh_capi.cpp): hand-made meshes against a plain numpy restatement of the rules (every
array and every count bit for bit: the restatement sums in the rules' order), the documented edges, the capped sphere and the
two spheres of the issue through the Poisson stub, the stub's two searches and its thread counts.  No GPU."""
import numpy as np
import pytest

from tests import test_poisson_cpu as psn
from tests.mesh_scenes import (ERR_ARG, NAN_BITS, OK, bits, build_stub, capped_sphere, cloud_near, fan, reference_finish, same, strip,
                               stub_finish, stub_sum, tetrahedron, tree_sum, two_spheres, two_tetrahedra)


@pytest.fixture(scope="module")
def ms(tmp_path_factory):
    return build_stub(tmp_path_factory.mktemp("mesh"))


@pytest.fixture(scope="module")
def ps(tmp_path_factory):
    return psn.build_stub(str(tmp_path_factory.mktemp("mesh_poisson") / "libpoissoncapi.so"))


@pytest.fixture(scope="module")
def capped(ms, ps):
    """the capped sphere, its mesh, r = 1.5 h and the stub's result at min_support 1, computed once"""
    xyz, v, t, h = capped_sphere(ps)
    rc, got = stub_finish(ms, xyz, None, v, t, 1.5 * h)
    assert rc == OK
    return xyz, v, t, 1.5 * h, got


@pytest.fixture(scope="module")
def spheres(ps):
    return two_spheres(ps)


HAND_MADE = {"tetrahedron": tetrahedron, "disjoint": lambda: two_tetrahedra(False), "shared": lambda: two_tetrahedra(True),
             "strip": lambda: strip(1000), "fan": lambda: fan(100)}


@pytest.mark.parametrize("name", list(HAND_MADE))
def test_hand_made_meshes_equal_the_numpy_restatement(ms, name):
    v, t = HAND_MADE[name]()
    xyz, rgb = cloud_near(v, 3)
    r = 0.012 if name in ("strip", "fan") else 0.3
    for kw in (dict(), dict(min_support=4), dict(min_support=0), dict(keep_largest=1), dict(min_component=5)):
        rc, got = stub_finish(ms, xyz, rgb, v, t, r, **kw)
        assert rc == OK
        same(got, reference_finish(xyz, rgb, v, t, r, **kw))
    rc, got = stub_finish(ms, xyz, rgb, v, t, r)
    assert got["summary"]["n_triangles"] == len(t) and got["summary"]["n_components"] == (2 if name == "disjoint" else 1)
    assert np.isfinite(got["normals"]).all() and np.allclose(np.linalg.norm(got["normals"].astype(np.float64), axis=1), 1.0, atol=1e-6)
    assert got["support"].min() >= 1 and (got["nearest"] >= 0).all()
    if name == "tetrahedron":
        assert abs(got["summary"]["volume"] - 1 / 6) < 1e-15 and abs(got["summary"]["area"] - (1.5 + np.sqrt(0.75))) < 1e-15
        # area-weighted and oriented outwards: vertex 0 sees the three coordinate faces, each of area 1/2
        assert np.allclose(got["normals"][0], -np.ones(3) / np.sqrt(3), atol=1e-7)
    if name == "fan":
        assert np.bincount(got["triangles"].reshape(-1))[0] == 100


def test_colours_follow_the_formula(ms):
    """one vertex, four coloured points inside the radius and one outside: w = (1 - d2 / r2)^2 over the points in grid order"""
    v, t = tetrahedron()
    r = 0.25
    xyz = np.float32([[0.1, 0, 0], [0, 0.2, 0], [0, 0, 0.05], [-0.1, -0.1, 0], [0.3, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]])
    rgb = np.uint32([0xFF0000, 0x00FF00, 0x0000FF, 0x808080, 0xFFFFFF, 0x010203, 0x040506, 0x070809])
    rc, got = stub_finish(ms, xyz, rgb, v, t, r)
    assert rc == OK and got["support"].tolist() == [4, 1, 1, 1] and got["nearest"].tolist() == [2, 5, 6, 7]
    assert got["rgb"][1:].tolist() == [0x010203, 0x040506, 0x070809]                 # a single point at distance 0: its colour
    r2 = float(np.float32(r * r))
    d2 = (xyz[:4].astype(np.float32) ** 2).sum(1, dtype=np.float32).astype(np.float64)
    w = (1 - d2 / r2) ** 2
    ch = [(rgb[:4] >> s) & 255 for s in (16, 8, 0)]
    want = [int((w * c).sum() / w.sum() + 0.5) for c in ch]
    have = [int(got["rgb"][0] >> s) & 255 for s in (16, 8, 0)]
    assert max(abs(a - b) for a, b in zip(have, want)) <= 1                            # (numpy's own sum order: a tie may round apart)
    assert got["nearest_d2"][0] == np.float32(0.05) ** 2
    same(got, reference_finish(xyz, rgb, v, t, r))
    rc, plain = stub_finish(ms, xyz, None, v, t, r)                                    # without colours: everything else the same
    assert rc == OK and plain["rgb"] is None and np.array_equal(plain["support"], got["support"])


def test_radius_and_support_edges(ms):
    v, t = tetrahedron()
    r = 0.5
    below = np.nextafter(np.float32(0.5), np.float32(0))
    # vertex 0: a point exactly at distance r (not counted) and one a float below (counted); the other vertices: 2 points each
    xyz = np.float32([[0.5, 0, 0], [0, below, 0], [1, 0, 0], [1, 0.01, 0], [0, 1, 0], [0, 1, 0.01], [0, 0, 1], [0.01, 0, 1]])
    assert np.float32(0.5) ** 2 == np.float32(r * r) and below * below < np.float32(r * r)
    rc, got = stub_finish(ms, xyz, None, v, t, r, min_support=0)
    assert rc == OK and got["support"].tolist() == [1, 2, 2, 2] and got["nearest"][0] == 1
    rc, got = stub_finish(ms, xyz, None, v, t, r, min_support=1)                       # support == min_support is kept
    assert rc == OK and got["summary"]["n_triangles"] == 4 and got["summary"]["n_unsupported_vertices"] == 0
    rc, got = stub_finish(ms, xyz, None, v, t, r, min_support=2)                       # ... and min_support - 1 is not
    assert rc == OK and got["summary"]["n_unsupported_vertices"] == 1 and got["triangles"].tolist() == [[0, 1, 2]]
    assert got["vertex_src"].tolist() == [1, 2, 3] and got["triangle_src"].tolist() == [3] and got["summary"]["n_trimmed_triangles"] == 3
    same(got, reference_finish(xyz, None, v, t, r, min_support=2))


def test_non_finite_far_and_degenerate_inputs(ms):
    v, t = two_tetrahedra(False)
    xyz, rgb = cloud_near(v, 5)
    xyz[3] = np.nan                                                                     # a NaN cloud point is nobody's support
    xyz[7, 1] = np.inf
    vb = v.copy()
    vb[4, 0] = np.nan                                                                   # the second tetrahedron loses a vertex
    vb[5, 2] = -np.inf
    for kw in (dict(min_support=0), dict(min_support=1)):                               # min_support 0 keeps everything finite, no more
        rc, got = stub_finish(ms, xyz, rgb, vb, t, 0.3, **kw)
        assert rc == OK and got["summary"]["n_unsupported_vertices"] == 2 and got["summary"]["n_triangles"] == 4
        assert not np.isin([4, 5], got["vertex_src"]).any() and np.isfinite(got["vertices"]).all()
        same(got, reference_finish(xyz, rgb, vb, t, 0.3, **kw))
    rc, none = stub_finish(ms, xyz, rgb, v, t, 0.3, min_support=0)
    assert rc == OK and none["summary"]["n_triangles"] == 8 and not np.isin([3, 7], none["nearest"]).any()
    far = np.concatenate([v, np.float32([[1e6, -1e6, 1e6]])])                           # a vertex 1e6 away finds nothing
    tf = np.concatenate([t, np.int32([[0, 1, 8]])])
    for search in (1, 2):
        rc, got = stub_finish(ms, xyz, rgb, far, tf, 0.3, min_support=0, search=search)
        assert rc == OK and got["support"][8] == 0 and got["nearest"][8] == -1 and np.isinf(got["nearest_d2"][8]) and got["rgb"][8] == 0
        same(got, reference_finish(xyz, rgb, far, tf, 0.3, min_support=0))
    rc, got = stub_finish(ms, xyz, rgb, far, tf, 0.3)
    assert rc == OK and got["summary"]["n_vertices"] == 8 and got["summary"]["n_trimmed_triangles"] == 1
    rep = np.concatenate([t, np.int32([[0, 0, 1], [2, 3, 2], [1, 1, 1]])])              # repeated indices never survive
    rc, got = stub_finish(ms, xyz, rgb, v, rep, 0.3, min_support=0)
    assert rc == OK and got["summary"]["n_trimmed_triangles"] == 3 and np.array_equal(got["triangles"], t)
    flat = np.float32([[0, 0, 0], [1, 0, 0], [2, 0, 0]])                                # a triangle without area: a NaN normal
    rc, got = stub_finish(ms, flat, None, flat, np.int32([[0, 1, 2]]), 0.3)
    assert rc == OK and (bits(got["normals"]) == NAN_BITS).all() and got["summary"]["area"] == 0.0
    same(got, reference_finish(flat, None, flat, np.int32([[0, 1, 2]]), 0.3))


def test_tiny_inputs_and_refusals(ms):
    v, t = tetrahedron()
    xyz, rgb = cloud_near(v, 6)
    for nv, nt in ((0, 0), (1, 0), (4, 0), (3, 1), (4, 1)):
        tt = np.int32([[0, 2, 1]])[:nt]
        rc, got = stub_finish(ms, xyz, rgb, v[:nv], tt, 0.3)
        assert rc == OK and got["summary"]["n_triangles"] == nt and got["summary"]["n_vertices"] == 3 * nt
        same(got, reference_finish(xyz, rgb, v[:nv], tt, 0.3))
    for cloud in (np.zeros((0, 3), np.float32), np.full((3, 3), np.nan, np.float32)):   # no finite point: an empty output
        for m in (0, 1):
            rc, got = stub_finish(ms, cloud, None, v, t, 0.3, min_support=m)
            assert rc == OK and got["summary"]["n_vertices"] == 0 and got["summary"]["n_unsupported_vertices"] == 4
            same(got, reference_finish(cloud, None, v, t, 0.3, min_support=m))
    for n in (1, 2):
        rc, got = stub_finish(ms, xyz[:n], rgb[:n], v, t, 5.0)
        assert rc == OK and (got["support"] == n).all() and got["summary"]["n_triangles"] == 4
        same(got, reference_finish(xyz[:n], rgb[:n], v, t, 5.0))
    assert stub_finish(ms, xyz, rgb, v, np.int32([[0, 1, 4]]), 0.3)[0] == ERR_ARG      # an index out of range
    assert stub_finish(ms, xyz, rgb, v, np.int32([[0, -1, 2]]), 0.3)[0] == ERR_ARG
    for r in (0.0, -1.0, np.nan, np.inf):
        assert stub_finish(ms, xyz, rgb, v, t, r)[0] == ERR_ARG
    for kw in (dict(min_support=-1), dict(min_component=-1), dict(keep_largest=-1)):
        assert stub_finish(ms, xyz, rgb, v, t, 0.3, **kw)[0] == ERR_ARG


@pytest.mark.parametrize("nt", [255, 256, 257])
def test_area_and_volume_are_the_tree_sums(ms, nt):
    v, t = strip(nt)
    xyz, _ = cloud_near(v, nt)
    rc, got = stub_finish(ms, xyz, None, v, t, 0.012)
    assert rc == OK and got["summary"]["n_triangles"] == nt
    p = got["vertices"].astype(np.float64)[got["triangles"]]
    cr = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
    area = 0.5 * np.sqrt((cr[:, 0] * cr[:, 0] + cr[:, 1] * cr[:, 1]) + cr[:, 2] * cr[:, 2])
    bc = np.cross(p[:, 1], p[:, 2])
    vol = ((p[:, 0, 0] * bc[:, 0] + p[:, 0, 1] * bc[:, 1]) + p[:, 0, 2] * bc[:, 2]) / 6.0
    assert got["summary"]["area"] == tree_sum(area) == stub_sum(ms, area) and got["summary"]["volume"] == tree_sum(vol) == stub_sum(ms, vol)
    assert abs(got["summary"]["area"] - area.sum()) < 1e-12


def test_component_filters(ms):
    v, t = two_tetrahedra(False)                                                         # two components of 4 triangles: ids 0 and 4
    xyz, rgb = cloud_near(v, 7)
    rc, got = stub_finish(ms, xyz, rgb, v, t, 0.3, keep_largest=1)                       # equal sizes: the lower id wins
    assert rc == OK and got["summary"]["n_components"] == 2 and got["summary"]["n_components_kept"] == 1
    assert got["vertex_src"].tolist() == [0, 1, 2, 3] and got["triangle_src"].tolist() == [0, 1, 2, 3]
    for k in (2, 3, 100):                                                                # keep_largest at and above the component count
        rc, got = stub_finish(ms, xyz, rgb, v, t, 0.3, keep_largest=k)
        assert rc == OK and got["summary"]["n_components_kept"] == 2 and got["summary"]["n_triangles"] == 8
    big = np.concatenate([t, np.int32([[4, 5, 6]])])                                     # the second component: 5 triangles
    rc, got = stub_finish(ms, xyz, rgb, v, big, 0.3, keep_largest=1)
    assert rc == OK and got["vertex_src"].tolist() == [4, 5, 6, 7] and got["summary"]["n_triangles"] == 5
    for m, kept in ((4, 2), (5, 1), (6, 0)):                                             # min_component_triangles equal to a size keeps it
        rc, got = stub_finish(ms, xyz, rgb, v, big, 0.3, min_component=m)
        assert rc == OK and got["summary"]["n_components_kept"] == kept, m
        same(got, reference_finish(xyz, rgb, v, big, 0.3, min_component=m))
    rc, got = stub_finish(ms, xyz, rgb, v, big, 0.3, min_component=5, keep_largest=2)
    assert rc == OK and got["summary"]["n_components_kept"] == 1 and got["summary"]["n_triangles"] == 5
    sv, st = two_tetrahedra(True)                                                        # a shared vertex joins them
    sx, sc = cloud_near(sv, 8)
    rc, got = stub_finish(ms, sx, sc, sv, st, 0.3, keep_largest=1)
    assert rc == OK and got["summary"]["n_components"] == 1 and got["summary"]["n_triangles"] == 8
    # the trim can split a component: the shared vertex unsupported leaves one triangle of each tetrahedron, ids 0 and 4
    far = sx[np.linalg.norm(sx - sv[3], axis=1) > 0.2]
    rc, got = stub_finish(ms, far, None, sv, st, 0.1)
    assert rc == OK and got["summary"]["n_unsupported_vertices"] == 1 and got["summary"]["n_components"] == 2
    same(got, reference_finish(far, None, sv, st, 0.1))


def test_capped_sphere(ms, capped):
    xyz, v, t, r, got = capped
    s = got["summary"]
    print(f"capped sphere: {s}")
    assert s["n_vertices_in"] == len(v) and s["n_components"] == 1 and s["n_components_kept"] == 1          # the output is one component
    assert (got["vertices"][:, 2] < 0.5 + r).all()                                       # M2: no point above z = 0.5
    low = (v[t][:, :, 2] < 0.5 - r).all(1)                                               # far below the rim: every one survives
    assert low.sum() > 10_000 and np.isin(np.flatnonzero(low), got["triangle_src"]).all()
    rc, all_v = stub_finish(ms, xyz, None, v, t, r, min_support=0)
    assert rc == OK and all_v["summary"]["n_triangles"] == len(t)
    least = all_v["support"][np.unique(t[low])].min()
    cap = (all_v["support"] == 0).sum()
    above = v[:, 2] >= 0.5 + r
    print(f"capped sphere: {low.sum()} triangles below the rim, least support among their vertices {least}, {cap} vertices with support 0, "
          f"{above.sum()} vertices at z >= 0.5 + r")
    assert low.sum() == 16268 and least == 28 and s["n_unsupported_vertices"] == cap
    assert above.sum() == 1189 and (all_v["support"][above] == 0).all()                   # the cap no point supports
    for m in (3, 5):
        rc, g = stub_finish(ms, xyz, None, v, t, r, min_support=m)
        assert rc == OK and np.isin(np.flatnonzero(low), g["triangle_src"]).all() and g["summary"]["n_components_kept"] >= 1
    assert np.array_equal(got["vertices"], v[got["vertex_src"]]) and np.array_equal(got["vertex_src"][got["triangles"]], t[got["triangle_src"]])
    n = got["normals"].astype(np.float64)                                                # the normals point away from the centre
    assert np.isfinite(n).all() and ((n * got["vertices"]).sum(1) > 0).all()


def test_two_spheres(ms, spheres):
    xyz, v, t, h = spheres
    r = 1.5 * h
    rc, both = stub_finish(ms, xyz, None, v, t, r)
    assert rc == OK and both["summary"]["n_components"] == 2 and both["summary"]["n_triangles"] == len(t)
    rc, a = stub_finish(ms, xyz, None, v, t, r, keep_largest=1)
    rc2, b = stub_finish(ms, xyz, None, v, t, r, min_component=1000)
    assert rc == OK and rc2 == OK
    same(a, b)
    big = a["summary"]["n_triangles"]
    print(f"two spheres: components of {big} and {len(t) - big} triangles")
    assert a["summary"]["n_components_kept"] == 1 and big == 12576 and len(t) - big == 408 and (a["vertices"][:, 0] < 1.2).all()
    psn.check_closed_oriented(a["vertices"], a["triangles"], 2)
    vol = psn.signed_volume(a["vertices"], a["triangles"])
    assert abs(a["summary"]["volume"] - vol) <= 1e-12 * abs(vol) and abs(vol - 4 / 3 * np.pi) < 0.05 * 4 / 3 * np.pi


def test_searches_and_thread_counts_do_not_change_a_bit(ms, capped):
    xyz, v, t, r, _ = capped
    rgb = np.random.default_rng(9).integers(0, 1 << 24, len(xyz), dtype=np.uint32)
    rc, first = stub_finish(ms, xyz, rgb, v, t, r, search=2, threads=1)
    assert rc == OK
    for search, threads in ((2, 3), (2, 16), (1, 16)):
        rc, got = stub_finish(ms, xyz, rgb, v, t, r, search=search, threads=threads)
        assert rc == OK
        same(got, first)
