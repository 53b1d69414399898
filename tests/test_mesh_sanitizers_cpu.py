"""CPU: AddressSanitizer + UBSan run of the mesh-finishing header's host build (tests/stub/mesh_capi.cpp with its driver, a
stand-alone program run as a child process): a sphere of 4 609 triangles (one with a repeated index, a NaN and an infinite
vertex) against a coloured cloud on its lower part with NaN and infinite rows, by both searches at 1 and 16 threads, without
colours, without trimming, with a blob beside it under the component filters, a tetrahedron, a vertex 1e6 away, the empty
cloud, the empty mesh, a mesh without a triangle, a cloud of one point and the refusals.  Host code only: sanitizers do not
run on the GPU."""
import os
import subprocess

from tests.mesh_scenes import STUB


def test_mesh_under_asan_ubsan(tmp_path):
    exe = str(tmp_path / "mesh_asan")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++14", "-ffp-contract=off", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=undefined", "-DMESH_MAIN", "-o", exe, STUB])
    r = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert r.returncode == 0, r.stderr[-3000:]
    assert "runtime error" not in r.stderr and r.stdout.startswith("sphere: search 1 threads 1 in 2352 4609 out ") and r.stdout.endswith("done\n")
    lines = r.stdout.split("\n")
    tails = {l.split(" in ", 1)[1] for l in lines if l.startswith("sphere: ")}
    assert r.stdout.count("sphere: ") == 4 and len(tails) == 1                       # the searches and the thread counts agree
    assert " components 2 kept 2 " in lines[6] and " components 2 kept 1 " in lines[7] and " components 2 kept 1 " in lines[8]
    for k in (7, 8):                                                                  # the blob gone: the sphere's mesh and sums
        assert lines[k].split(" area ")[1] == lines[0].split(" area ")[1]
        assert lines[k].split(" out ")[1].split(" unsupported ")[0] == lines[0].split(" out ")[1].split(" unsupported ")[0]
    assert "tetrahedron: search 0 threads 1 in 4 4 out 4 4 unsupported 0 trimmed 0 components 1 kept 1 area 2.3660254 volume 0.166666667 " in r.stdout
    assert "far vertex: search 2 threads 1 in 5 5 out 4 4 unsupported 1 trimmed 1 " in r.stdout
    assert "empty cloud: search 0 threads 1 in 4 4 out 0 0 unsupported 4 trimmed 4 components 0 kept 0 area 0 volume 0 " in r.stdout
    assert "no triangle: search 0 threads 1 in 4 0 out 0 0 unsupported 0 trimmed 0 " in r.stdout and "refusals -3 -3 -3 -3 -3 -3\n" in r.stdout
