"""Builds libsfmhip.so (HIP kernels + C ABI, gfx950 only) in-tree with hipcc.

hipcc cross-compiles without a GPU, so this runs in the dev container; the .so travels to the
GPU box with the repository snapshot.
"""
import os
import shutil
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
SO = os.path.join(HERE, "libsfmhip.so")
# per-source floating-point contraction: the matcher's exact kernel, the triangulation and the pose step restate
# OpenCV's operation order, the dense-cloud step PCL's (no compiler-chosen FMAs); the BA kernels are tolerance-level f64
# and want v_fma_f64 -- "fast-honor-pragmas", not "fast": the one function that must NOT contract, the trust-region decision
# lm_decide (the same bits on the host and on the device), says so with a pragma, which plain "fast" ignores
SOURCES = {"context.hip": "off", "match.hip": "off", "triangulate.hip": "off", "incremental.hip": "off",
           "score.hip": "off", "pose.hip": "off", "pnp.hip": "off", "cloud.hip": "off", "cloud_filter.hip": "off", "mls.hip": "off", "register.hip": "off", "align.hip": "off", "segment.hip": "off", "poisson.hip": "off", "mesh.hip": "off", "dendro.hip": "off", "ground.hip": "off", "trees.hip": "off", "terrain.hip": "off", "crowns.hip": "off", "tracks.hip": "off", "verify.hip": "off", "mvs.hip": "off", "undistort.hip": "off", "sift.hip": "off", "ba.hip": "fast-honor-pragmas", "probe.hip": "off"}
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc():
    for c in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found")


def needs_build():
    if not os.path.exists(SO):
        return True
    t = os.path.getmtime(SO)
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC)] + [os.path.join(HERE, "..", "include", "sfmhip.h")]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    if not force and not needs_build():
        return SO
    objdir = os.path.join(HERE, "build")
    os.makedirs(objdir, exist_ok=True)
    objs, procs = [], []
    for name, contract in SOURCES.items():
        src = os.path.join(CSRC, name)
        obj = os.path.join(objdir, name.replace(".hip", ".o"))
        objs.append(obj)
        hdrs = [os.path.join(CSRC, h) for h in os.listdir(CSRC) if h.endswith(".h")]  # (every header of csrc/: common.h, cloud_grid.h, the arithmetic headers, the BA planners)
        if not force and os.path.exists(obj) and os.path.getmtime(obj) >= max(
                [os.path.getmtime(src), os.path.getmtime(os.path.join(HERE, "..", "include", "sfmhip.h"))] +
                [os.path.getmtime(h) for h in hdrs]):
            continue
        cmd = [_hipcc()] + FLAGS + [f"-ffp-contract={contract}", "-c", src, "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((cmd, subprocess.Popen(cmd)))
    for cmd, p in procs:
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, cmd)
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", SO] + objs
    if verbose:
        print(" ".join(cmd))
    subprocess.check_call(cmd)
    return SO


def build_ba_variant(name, defines, force=False):
    """libsfmhip_<name>.so: the library with ba.hip compiled under extra -D switches, every other object shared with the product
    build (diagnostic and A/B builds: loaded through SFMHIP_SO, never by the product)."""
    build()
    objdir = os.path.join(HERE, "build")
    so = os.path.join(HERE, f"libsfmhip_{name}.so")
    deps = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith((".h", ".hip"))]
    if not force and os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(d) for d in deps):
        return so
    obj = os.path.join(objdir, f"ba_{name}.o")
    subprocess.check_call([_hipcc()] + FLAGS + [f"-ffp-contract={SOURCES['ba.hip']}"] + list(defines) +
                          ["-c", os.path.join(CSRC, "ba.hip"), "-o", obj])
    objs = [os.path.join(objdir, n.replace(".hip", ".o")) for n in SOURCES if n != "ba.hip"] + [obj]
    subprocess.check_call([_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", so] + objs)
    return so


def build_timeout_diag(force=False):
    """Two diagnostic builds of the library in which one hand-off never arrives (test infrastructure: tests/test_gpu_geometry.py
    checks what the solver reports then; loaded through SFMHIP_SO, never by the product): libsfmhip_dbg_breakfront.so -- a child
    front of the tree never raises its flag in the one-launch form (-DSFM_FRONT_BREAK_HANDOFF) -- and libsfmhip_dbg_breakchol.so --
    an LDS hand-off inside chol_step2 never arrives (-DSFM_CHOL_BREAK_HANDOFF)."""
    return [build_ba_variant("dbg_breakfront", ["-DSFM_FRONT_BREAK_HANDOFF"], force),
            build_ba_variant("dbg_breakchol", ["-DSFM_CHOL_BREAK_HANDOFF"], force)]


def build_host_demo(force=False):
    """C++ host mirror (Sfm.h / BundleAdjustment.h call surface) + its self-test executable."""
    host = os.path.join(CSRC, "host")
    exe = os.path.join(HERE, "sfm_host_selftest")
    return _build_host_exe(exe, ("Sfm.cpp", "SfmIO.cpp", "BundleAdjustment.cpp", "selftest.cpp"), force)


def build_ba_demo(force=False):
    """BundleAdjustment::adjustBundle on a problem of any size in the reference's containers (tests/test_gpu_host_cpp.py: the
    write-back-only-on-CONVERGENCE policy at cfg4 size)."""
    return _build_host_exe(os.path.join(HERE, "sfm_ba_selftest"), ("Sfm.cpp", "SfmIO.cpp", "BundleAdjustment.cpp", "ba_selftest.cpp"), force)


def build_io_demo(force=False):
    """The I/O self-test of the host mirror (imagesLOAD / getCameraMatrix / PMVS2).
    Runs without a GPU: the host classes open the device only when a matching / BA call needs it."""
    return _build_host_exe(os.path.join(HERE, "sfm_io_selftest"), ("Sfm.cpp", "SfmIO.cpp", "BundleAdjustment.cpp", "io_selftest.cpp"), force)


def build_pose_demo(force=False):
    """The base reconstruction of the host mirror (baseReconstruction: findBestPair, getCameraPose over the map in one
    sfmhip_essential_pose call, triangulateViews) followed by adjustCurrentBundle, on a directory of frames (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_pose_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmPose.cpp", "BundleAdjustment.cpp", "pose_selftest.cpp"), force,
                           std="c++17")  # (SfmPose.cpp includes ../pose.h, whose hypot restatement has hex float literals)


def build_incr_demo(force=False):
    """The incremental reconstruction of the host mirror: baseReconstruction, then addMoreViews (findCameraPosePNP over
    sfmhip_pnp_ransac, triangulateViews, mergeNewPoints, adjustCurrentBundle per added view) on a scene file of points and
    matches or on a directory of frames (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_incr_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmPose.cpp", "SfmIncremental.cpp", "BundleAdjustment.cpp", "incr_selftest.cpp"),
                           force, std="c++17")


def build_tracks_demo(force=False):
    """The track consolidation of the host mirror: baseReconstruction, addMoreViews, then consolidateTracks (sfmhip_tracks_build /
    sfmhip_tracks_triangulate over all pairs of the registered views) and one more adjustBundle, on incr_selftest's inputs; writes
    the cloud before and after the consolidation (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_tracks_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmPose.cpp", "SfmIncremental.cpp", "SfmTracks.cpp", "BundleAdjustment.cpp",
                            "tracks_selftest.cpp"), force, std="c++17")


def build_cloud_demo(force=False):
    """map3D's steps 8-10 in the host mirror (convertPLYtoPCD, loadPCDFile, cloudPointFilter, removePoints and create_mesh's
    normals, all on the unfiltered cloud as the reference calls them) on a PLY file (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_cloud_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "cloud_selftest.cpp"), force)


def build_cloud_filter_demo(force=False):
    """pcl::VoxelGrid and pcl::StatisticalOutlierRemoval as pcllite.h mirrors them, then computeNormals, on a PCD file; writes the
    kept points and their normals as a binary PCD (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_cloud_filter_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "cloud_filter_selftest.cpp"), force)


def build_smooth_demo(force=False):
    """The smoothing pass in front of create_mesh in the host mirror (StructFromMotion::smoothCloud over pcl::MovingLeastSquares as
    pcllite.h mirrors it, then create_mesh with a smoothing radius: MLS, normals and Poisson on one device cloud) on a PCD; writes
    the smoothed points with their normals as a binary PCD and the meshes as binary PLYs (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_smooth_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "smooth_selftest.cpp"), force)


def build_mesh_demo(force=False):
    """map3D's last call in the host mirror (create_mesh: the normals, their flip, then Poisson at depth 7) on a MAP3D.pcd;
    writes the mesh as a binary PLY (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_mesh_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "mesh_selftest.cpp"), force)


def build_mesh_finish_demo(force=False):
    """create_mesh on a coloured cloud in the host mirror: the normals, Poisson at depth 7, then StructFromMotion::finishMesh (the
    trim of unsupported surface, per-vertex colours and normals) on a PCD; writes the finished mesh as a binary PLY with normals
    and colours (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_mesh_finish_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "mesh_finish_selftest.cpp"), force)


def build_dense_demo(force=False):
    """map3D's step 7 in the host mirror (StructFromMotion::densify: sfmhip_mvs_run over the registered views) on a directory
    of frames, a calibration file and a file of poses and sparse points; writes denseCloud's PLY (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_dense_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmDense.cpp", "BundleAdjustment.cpp", "dense_selftest.cpp"), force)


def build_segment_demo(force=False):
    """The two steps after map3D in the host mirror (Segmentation::color_based_growing_segmentation, then
    Dendrometry::estimate) on a MAP3D.pcd with colours (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_segment_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "BundleAdjustment.cpp", "Segmentation.cpp", "DendrometryE.cpp", "segment_selftest.cpp"),
                           force)


def build_dendro_demo(force=False):
    """The measurement the reference's Dendrometry leaves blank, in the host mirror (Dendrometry::measure and estimateTree over
    sfmhip_cloud_dendrometry) on a MAP3D.pcd, optionally on one cluster of the colour segmentation (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_dendro_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "BundleAdjustment.cpp", "Segmentation.cpp", "DendrometryE.cpp", "dendro_selftest.cpp"),
                           force)


def build_registration_demo(force=False):
    """Two reconstructions of one plot in two gauges brought together in the host mirror (pcl::IterativeClosestPointWithScale,
    StructFromMotion::registerCloud, pcl::transformPointCloud, sfmhip_cloud_concat, the voxel grid and Dendrometry::estimatePlot
    on the sum); makes its own plots (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_registration_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "Segmentation.cpp", "DendrometryE.cpp",
                            "registration_selftest.cpp"), force)


def build_align_demo(force=False):
    """Two reconstructions of one plot in unrelated gauges brought together without a starting guess in the host mirror
    (computeGroundPlane on each, StructFromMotion::alignPlots, then registerCloud from its result); makes its own plots
    (needs the GPU)."""
    return _build_host_exe(os.path.join(HERE, "sfm_align_selftest"),
                           ("Sfm.cpp", "SfmIO.cpp", "SfmCloud.cpp", "BundleAdjustment.cpp", "Segmentation.cpp", "DendrometryE.cpp",
                            "align_selftest.cpp"), force)


def _build_host_exe(exe, files, force, std="c++14"):
    host = os.path.join(CSRC, "host")
    srcs = [os.path.join(host, f) for f in files]
    deps = srcs + [os.path.join(host, f) for f in os.listdir(host) if f.endswith(".h")] + [os.path.join(CSRC, h) for h in ("pose.h", "pnp.h", "camera.h", "jacobi.h", "ransac_host.h")]
    if not force and os.path.exists(exe) and all(os.path.getmtime(exe) >= os.path.getmtime(s) for s in deps):
        return exe
    build()
    cmd = ["g++", "-O2", f"-std={std}", "-pthread", "-I", os.path.join(HERE, "..", "include"), "-I", host, "-o", exe] + srcs + \
          ["-L", HERE, "-lsfmhip", "-Wl,-rpath,$ORIGIN"]
    subprocess.check_call(cmd)
    return exe


def build_rccl(force=False):
    """libsfmhip_rccl.so: the native RCCL binding of the sharded BA (include/sfmhip_rccl.h)."""
    src = os.path.join(CSRC, "rccl", "sfmhip_rccl.cpp")
    so = os.path.join(HERE, "libsfmhip_rccl.so")
    if not force and os.path.exists(so) and os.path.getmtime(so) >= max(os.path.getmtime(src), os.path.getmtime(SO)):
        return so
    build()
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-x", "c++", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(rocm, "include"),
           "-o", so, src, "-L", HERE, "-lsfmhip", "-L", os.path.join(rocm, "lib"), "-lrccl", "-lamdhip64",
           "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(rocm, "lib")]
    subprocess.check_call(cmd)
    exe = os.path.join(HERE, "sfm_rccl_selftest")
    subprocess.check_call(["g++", "-O2", "-std=c++14", "-o", exe, os.path.join(CSRC, "rccl", "rccl_selftest.cpp"), "-L", HERE,
                           "-lsfmhip_rccl", "-lsfmhip", "-Wl,-rpath,$ORIGIN", "-Wl,-rpath," + os.path.join(rocm, "lib")])
    return so


if __name__ == "__main__":
    print(build(force=True, verbose=True))
