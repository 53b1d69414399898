// Sfm.h -- the hot-path part of the reference's StructFromMotion (include/Sfm.h:15-35,89,
// 107-117): same member names, same method signatures.  The incremental loop (addMoreViews, findCameraPosePNP over
// sfmhip_pnp_ransac) is in SfmIncremental.cpp; the Poisson mesh and the viewers are out of scope;
// map3D's step 10 filters and normals are in SfmCloud.cpp.
#pragma once
#include <map>
#include <set>
#include <string>
#include "BundleAdjustment.h"
#include "pcllite.h"
#include "sfmhip.h"

class StructFromMotion {
 private:
  std::vector<cv::Matx34d> nCameraPoses;
  Intrinsics cameraMatrix;
  float NN_MATCH_RATIO;
  std::vector<std::vector<cv::KeyPoint>> imagesKeypoints;
  std::vector<cv::Mat> imagesDescriptors;
  std::vector<std::vector<cv::Point2d>> imagesPts2D;
  int detector;
  std::set<int> nDoneViews;  // reference include/Sfm.h:24-25
  std::set<int> nGoodViews;
  // image I/O state, reference include/Sfm.h:18-23
  std::vector<cv::Mat> mColorImages;
  std::vector<cv::Mat> mGrayImages;
  std::vector<cv::Mat> nImages;
  std::vector<std::string> nImagesPath;
  std::string pathImages;
  // pair-match cache: getMatching is a pure function of two descriptor
  // matrices and the reference calls it ~1.5 N^2 times for N(N-1)/2 distinct pairs
  std::map<std::pair<int, int>, Matching> pairCache;
  bool pairCacheOn;
  // descriptors resident in HBM + a reusable one-pair plan: a getMatching call that misses the
  // cache costs one kernel sequence instead of two uploads and a dozen allocations
  sfmhip_imageset* devSet;
  sfmhip_matchplan* devPlan;
  void releaseDeviceSet();
  // descriptor rows that extractFeature left in HBM (sfmhip_sift_batch), image by image (nullptr: host rows only).
  // The matcher adopts them in place; imagesDescriptors[i] then carries the shape only until descriptors() is asked.
  std::vector<void*> devDescriptors;
  void releaseDeviceDescriptors();
  int uploadOrAdopt(sfmhip_imageset* set, int image);
  // the pose step: one pair's sfmhip_essential_pose outcome, and the part of getCameraPose after it
  struct PoseOutcome {
    double E[9], R[9], T[3];
    int32_t inliers, n_good;
    std::vector<uint8_t> mask;
  };
  bool essentialPoses(const std::vector<Points2d>& left, const std::vector<Points2d>& right, std::vector<PoseOutcome>& out);
  bool cameraPoseFrom(const int& idx_query, const int& idx_train, const Matching& matches, const Points2d& alignedLeft,
                      const Points2d& alignedRight, const PoseOutcome* outcome, cv::Matx34d& Pleft, cv::Matx34d& Pright);

 public:
  std::vector<Point3D> nReconstructionCloud;

  StructFromMotion() : NN_MATCH_RATIO(0.8f), detector(1), pairCacheOn(false), devSet(nullptr), devPlan(nullptr) {}
  ~StructFromMotion() {
    releaseDeviceSet();
    releaseDeviceDescriptors();
  }
  StructFromMotion(const StructFromMotion&) = delete;
  StructFromMotion& operator=(const StructFromMotion&) = delete;

  // reference include/Sfm.h:89, src/Sfm.cpp:590-608
  void getMatching(const int& queryImage, const int& trainImage, Matching* goodMatches);
  // reference include/Sfm.h:107-111, src/Sfm.cpp:694-711
  void AlignedPointsFromMatch(const Points2d& queryImg, const Points2d& trainImg, const Matching& matches,
                              Points2d& alignedL, Points2d& alignedR);
  void AlignedPoints(const Points2d& queryImg, const Points2d& trainImg, const Matching& matches, Points2d& alignedL,
                     Points2d& alignedR, std::vector<int>& idLeftOrigen, std::vector<int>& idRightOrigen);
  // reference include/Sfm.h:115-117, src/Sfm.cpp:804-878
  bool triangulateViews(const Points2d& left, const Points2d& right, const cv::Matx34d& P1, const cv::Matx34d& P2,
                        const Matching& matches, const Intrinsics& matrixK, const std::pair<int, int>& imagePair,
                        std::vector<Point3D>& pointcloud);
  // reference include/Sfm.h:135-137, src/Sfm.cpp:1011-1095: best done view by match count, then the
  // 2D-3D association of the cloud against that view's matches
  void find2D3DMatches(const int& NEW_VIEW, std::vector<cv::Point3d>& points3D, std::vector<cv::Point2d>& points2D,
                       Matching& bestMatches, int& DONEVIEW);
  // reference include/Sfm.h:150, src/Sfm.cpp:1212-1244
  void mergeNewPoints(const std::vector<Point3D>& newPointCloud);
  // The all-pairs loop of findBestPair (src/Sfm.cpp:511-515) as ONE batched device launch; fills
  // the pair cache that getMatching then serves from (identical results, pair order q<t).
  void matchAllPairs();
  // reference include/Sfm.h:83, src/Sfm.cpp:499-585: the all-pairs matching (matchAllPairs: one batched launch),
  // then for every pair with >= 120 matches the pose-inlier ratio of cv::findEssentialMat(RANSAC, 0.999, 1.0)
  // (sfmhip_score_essential, all pairs in one call), collected in the map keyed by that float: ascending, equal keys
  // overwrite; the homography inlier count the reference prints next to it (:545,567) comes from
  // sfmhip_score_homography, all pairs in one call.  Not mirrored: the drawMatches / imshow / waitKey(100) per pair.
  std::map<float, std::pair<int, int>> findBestPair();
  // reference include/Sfm.h:137, src/Sfm.cpp:667-689: cv::findHomography(RANSAC, 0.004 * maxVal) inlier count of one pair
  int findHomographyInliers(const int& idx_query, const int& idx_train, const Matching& matches);
  // reference src/Sfm.cpp:883-888 is a stub whose call names a member that no longer exists;
  // wired here with imagesPts2D, the member of the required type
  void adjustCurrentBundle();

  // ---- the pose step of baseReconstruction (csrc/host/SfmPose.cpp; sfmhip_essential_pose)
  // reference include/Sfm.h:121, src/Sfm.cpp:408-492: findBestPair, then ONE sfmhip_essential_pose call over every entry
  // of its map (each pair's outcome is independent of the others), then the map in ascending key order: the first pair
  // whose pose passes is triangulated and seeds nReconstructionCloud, nCameraPoses, nDoneViews and nGoodViews.  Prints
  // the reference's lines for the pairs it would have tried (not mirrored: the drawMatches / imshow / waitKey).
  // DEVIATION: where RANSAC returns no model the reference throws inside decomposeEssentialMat; the mirror writes a line
  // to stderr and goes on with the next pair.  Returns true, like the reference, once findBestPair's map is non-empty
  // and the batched pose call ran; false when the map is empty or that call failed (a device error).
  bool baseReconstruction();
  // reference include/Sfm.h:168, src/Sfm.cpp:713-789: prunedMatchingWithHomography (printed only, SURVEY.md appendix B
  // quirk 7), findEssentialMat(K, RANSAC, 0.999, 1.0) -> recoverPose(E, ..., fx, (cx, cy), mask) on the unpruned
  // matches (sfmhip_essential_pose), CheckCoherentRotation; false when K is empty, 7 or fewer points are aligned, RANSAC
  // finds no model (the deviation above) or the rotation check fails.  Pleft = [I|0], Pright = [R|T].  The pose comes
  // from AlignedPointsFromMatch(left, right, matches); the pruning reads the member imagesPts2D, as the reference's reads
  // imagesKeypoints.
  bool getCameraPose(const Intrinsics& intrinsics, const int& idx_query, const int& idx_train, const Matching& matches,
                     const Points2d& left, const Points2d& right, cv::Matx34d& Pleft, cv::Matx34d& Pright);
  // reference include/Sfm.h:103, src/Sfm.cpp:791-799: fabsf(determinante(R)) - 1.0 > 1e-07 fails (fabsf narrows to float)
  bool CheckCoherentRotation(cv::Mat& R);
  // reference include/Sfm.h:133, src/Sfm.cpp:1119-1131: Eigen::FullPivLU(R).determinant() of a 3 x 3 CV_64F
  double determinante(cv::Mat& relativeRotationCam);
  // reference include/Sfm.h:90, src/Sfm.cpp:610-662: the inliers of cv::findHomography(RANSAC, 2.5) on the keypoints
  // (sfmhip_score_homography, confidence 0.995, 2000 iterations); fewer than 4 matches: none
  void prunedMatchingWithHomography(const int& idx_query, const int& idx_train, const Matching& goodMatches,
                                    Matching* prunedMatch);
  // ---- the incremental loop (csrc/host/SfmIncremental.cpp; sfmhip_pnp_ransac)
  // reference include/Sfm.h:141-142, src/Sfm.cpp:1137-1210: refuses 7 or fewer points or lists of different length;
  // solvePnPRansac(K, dist, 1000 iterations, 0.006 * the largest 2-D coordinate, 0.99, CV_EPNP) = one sfmhip_pnp_ransac view
  // (its rules: include/sfmhip.h); when RANSAC returns no inliers (no model: rvec and T stay zero, as the
  // reference's freshly assigned outputs do) the points that project within 8 pixels form the inlier list; refuses
  // norm(T) > 200 and a rotation that fails CheckCoherentRotation; P = [R|T].
  // DEVIATION: the reference passes useExtrinsicGuess = true with an empty rvec; that is treated as no guess.
  bool findCameraPosePNP(const Intrinsics& intrinsics, const std::vector<cv::Point3d>& pts3D,
                         const std::vector<cv::Point2d>& pts2D, cv::Matx34d& P);
  // reference include/Sfm.h:125, src/Sfm.cpp:893-1006, line by line: each round proposes the neighbours i - 1 / i + 1 of the
  // done views (with the reference's quirks: |i - 1| for view 0 never arises, view nImages.size() is compared but cannot
  // exist, so the last view proposes one past the end), every proposed view is
  // marked done BEFORE its pose is tried, a posed view is triangulated against every good view (getMatching ->
  // triangulateViews -> mergeNewPoints), becomes good, and adjustCurrentBundle() runs.
  // DEVIATIONS: a proposed view outside [0, nImages.size()) is dropped (the reference would throw in .at()); the loop also
  // ends when a round proposes no new view (the reference would spin when a view can never be reached).
  bool addMoreViews();
  // ---- multi-view tracks (csrc/host/SfmTracks.cpp; sfmhip_tracks_*; no counterpart in the reference, whose
  // points keep the two views they were triangulated from).  One match plan over all pairs of nGoodViews -- on the resident
  // image set where the descriptors are there, else the pair cache / getMatching's lists --, the tracks of those lists with
  // >= max(2, minViews) views, one DLT point per track over nCameraPoses (6 px, as triangulateViews).  REPLACES
  // nReconstructionCloud by one Point3D per kept track with every view in idxImage / pt2D and returns the number of points;
  // on a device error the cloud stays as it is.  Nothing calls it by default.
  // verify: the lists first pass the two-view verification (sfmhip_matchplan_verify on the resident route, sfmhip_verify_lists
  // on the host-list route) with cameraMatrix.K over imagesPts2D, at its default options, and the tracks are
  // built from what it keeps; the last call's statistics are lastVerifyStats().  false: the call as it was.
  size_t consolidateTracks(int minViews = 2, bool verify = false);
  const sfmhip_verify_stats& lastVerifyStats() const { return verifyStats; }
  // the inlier list of the last findCameraPosePNP (the reference computes it and reads it nowhere)
  const std::vector<int>& lastPnpInliers() const { return pnpInliers; }
  const std::set<int>& doneViews() const { return nDoneViews; }
  const std::set<int>& goodViews() const { return nGoodViews; }

 private:
  std::vector<int> pnpInliers;
  sfmhip_verify_stats verifyStats = {0, 0, 0, 0, 0};

 public:
  // what the last baseReconstruction chose (pose_selftest): the pair, E, R, T, recoverPose's count and mask
  struct BasePose {
    int query = -1, train = -1, n_good = 0;
    double E[9] = {0}, R[9] = {0}, T[3] = {0};
    std::vector<uint8_t> mask;
  };
  const BasePose& basePose() const { return lastBasePose; }

 private:
  BasePose lastBasePose;

 public:

  // ---- detector / descriptor front end (csrc/host/SfmIO.cpp)
  // reference include/Sfm.h:85, src/Sfm.cpp:257-296: every gray image through getFeature (the imshow / waitKey(100) per
  // image are not mirrored)
  void extractFeature();
  // reference include/Sfm.h:81, src/Sfm.cpp:300-403: detector 1 = SIFT(0, 3, 0.04, 10, 1.6)->detectAndCompute on the
  // device (sfmhip_sift_detect_and_compute); detectors 2 (AKAZE) and 3 (ORB) are not built and leave the image's
  // containers empty with a message
  void getFeature(const cv::Mat& image, const int& numImage);
  // reference include/Sfm.h:95, src/Sfm.cpp:397-403
  void keypointstoPoints(std::vector<cv::KeyPoint>& keypoints, Points2d& points2D);
  void setKeypoints(int numImage, const float* kp, int n);
  const std::vector<std::vector<cv::KeyPoint>>& keypoints() const { return imagesKeypoints; }
  // (downloads the rows of images whose descriptors live in HBM only)
  const std::vector<cv::Mat>& descriptors();
  const std::vector<std::vector<cv::Point2d>>& points2D() const { return imagesPts2D; }

  // ---- I/O and interchange formats (csrc/host/SfmIO.cpp)
  // reference include/Sfm.h:77, src/Sfm.cpp:118-198: scan a directory for .jpg/.png, sort, decode to BGR,
  // x0.6 bilinear iff rows > 480 and cols > 640, colour + gray copies.  PNG and Huffman-coded 8-bit JPEG -- sequential and
  // progressive -- are decoded here (no OpenCV, no libpng / libjpeg; the JPEG path follows libjpeg's integer IDCT, fancy
  // upsampling and colour tables byte for byte, interleaved or one scan per component, any of the 1x1 / 2x1 / 1x2 / 2x2
  // samplings; a JPEG is turned as its EXIF orientation says, like cv::imread's default; PNG: Adam7 too); an arithmetic-coded,
  // lossless or 12-bit JPEG is reported and fails the load.
  bool imagesLOAD(const std::string& directoryPath);
  // reference include/Sfm.h:99, src/Sfm.cpp:203-252: the OpenCV FileStorage XML with Camera_Matrix and
  // Distortion_Coefficients.  Values are read as the numbers the file holds (the reference reads a `dt f`
  // matrix through at<double>); coefficient slots kept in file order.
  bool getCameraMatrix(const std::string str);
  // reference include/Sfm.h:179, src/Sfm.cpp:1246-1303: denseCloud/{visualize,txt,models}, options.txt,
  // visualize/%04d.jpg = a byte copy of the input file (what the reference's `cp -f` does; its imwrite
  // targets the command string and writes nothing), txt/%04d.txt = "CONTOUR" + K*P.  Does NOT run pmvs2.
  void PMVS2();
  // step 7 of map3D (reference src/Sfm.cpp:62-67: std::system("pmvs2 denseCloud/ options.txt")), csrc/host/SfmDense.cpp:
  // sfmhip_mvs_run over the registered views (nGoodViews) at level 1 and min_views 5 (options.txt's level and minImageNum;
  // rules and the deviations from pmvs2 in DESIGN.md f-10, parity UNPINNED).  A view's depth range is the smallest and the
  // largest depth of the sparse-cloud points it observes, widened by 25 %; a view with fewer than 8 such points is left
  // out.  Writes the binary little-endian PLY (x y z nx ny nz red green blue) that convertPLYtoPCD reads and returns the
  // point count (0: fewer than two usable views, a device error or an unwritable file, with a line on stderr).
  size_t densify(const std::string& plyPath = "denseCloud/models/options.txt.ply");
  // reference src/Sfm.cpp:69-81 (step 8 of map3D): denseCloud/models/options.txt.ply -> MAP3D.pcd.  The reference
  // does this with pcl::PLYReader + pcl::io::savePCDFile (ASCII, PointXYZRGB); here a PLY reader (ascii and
  // binary_little_endian; x y z [nx ny nz] [diffuse_]red green blue) and a PCD v0.7 ASCII writer in the layout PCL
  // 1.8 documents (FIELDS x y z rgb, rgb = the packed 0x00RRGGBB word printed as a float).  Returns the point count
  // (0 = "ply file is empty", the reference's failure case).  Not pinned against PCL: it is absent from the image.
  static size_t convertPLYtoPCD(const std::string& plyPath, const std::string& pcdPath);
  // ---- map3D step 10 on the dense cloud (csrc/host/SfmCloud.cpp; sfmhip_cloud_*, PCL parity UNPINNED: DESIGN.md f-6)
  // The three calls share one device upload and its grids while the cloud's points are unchanged (SfmCloud.cpp keeps
  // one handle, keyed by the points' count and a hash of their bytes).  The reference's step 10 passes the UNFILTERED
  // cloud to all three (src/Sfm.cpp:98-100); cloud_selftest.cpp reproduces that order.
  // reference include/Sfm.h:182, src/Sfm.cpp:1323-1332: PassThrough on x, limits (float) 0.003 and 0.83, inclusive;
  // non-finite points dropped; input order kept.  filterCloud takes the kept points, is_dense and the sensor origin of
  // `cloud`.
  void cloudPointFilter(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PointCloud<pcl::PointXYZ>::Ptr& filterCloud);
  // reference include/Sfm.h:184, src/Sfm.cpp:1334-1344: RadiusOutlierRemoval, radius 0.07, 150 neighbours: a point is
  // kept iff more than 150 finite points (itself included) lie at d2 < (float)(0.07 * 0.07); input order kept.
  void removePoints(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PointCloud<pcl::PointXYZ>::Ptr& filterCloud);
  // the first half of create_mesh (reference include/Sfm.h:186, src/Sfm.cpp:1346-1366): NormalEstimation with
  // setKSearch(10) towards the cloud's sensor origin, then every normal multiplied by -1.  normals has one entry per
  // point of `cloud` (NaN where PCL writes NaN).
  void computeNormals(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PointCloud<pcl::Normal>::Ptr& normals);
  // create_mesh (reference include/Sfm.h:186, src/Sfm.cpp:1346-1381): computeNormals (with its -1 flip), the cloud and
  // its normals concatenated, then pcl::Poisson with setDepth(7), setPointWeight(4), setScale(1.1) -- here
  // sfmhip_cloud_poisson on the same device cloud (a uniform 128^3 grid for PCL's octree, marching
  // tetrahedra for its cubes; parity UNPINNED).  Ignored PCL setters, having no counterpart: setSamplesPerNode(1),
  // setIsoDivide(8), setSolverDivide(8), setManifold(false), setOutputPolygons(false); setConfidence(1) has no effect on
  // unit normals.  The solve runs with cg_max_iter = 8 * 2^depth = 1024: the library's default of 4 * 2^depth = 512 steps
  // does not reach cg_rtol 1e-8 at depth 7 (a 200 k-point sphere takes 538); a solve that still ends at the cap is
  // reported on stderr with its residual.  mesh.cloud takes the vertices, mesh.polygons the triangles.  vizualizeMesh is
  // not built (GUI).
  void create_mesh(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PolygonMesh& mesh);
  // (ours) the pass the reference's create_mesh still names (`cloud_smoothed`, src/Sfm.cpp:1347-1383) and does
  // not run: pcl::MovingLeastSquares with search radius `radius` and the polynomial of `order` (0: the plane alone), normals
  // computed; smoothed takes the surviving points in input order.
  void smoothCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, double radius, int order, pcl::PointCloud<pcl::PointNormal>::Ptr& smoothed);
  // create_mesh with that pass in front: sfmhip_cloud_mls at order 2 and radius smooth_radius, then the normals (k = 10, towards
  // the sensor origin, times -1) and Poisson as above on the smoothed handle; the smoothed points never come to the host.
  void create_mesh(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, pcl::PolygonMesh& mesh, double smooth_radius);
  // (ours) the finishing of a mesh against the coloured cloud it was made from: sfmhip_cloud_mesh_finish (the
  // trim of the surface no point within opts.support_radius supports, the component filters, per-vertex colours and normals).
  // mesh is replaced by the finished mesh, mesh.colours and mesh.normals filled.  Returns the call's summary.
  sfmhip_mesh_finish_summary finishMesh(const pcl::PointCloud<pcl::PointXYZRGB>& cloud, pcl::PolygonMesh& mesh, const sfmhip_mesh_finish_opts& opts);
  // create_mesh on a coloured cloud (its sensor origin as the two-argument form takes it), then finishMesh with
  // support_radius = 1.5 cells of the Poisson cube -- the half-width of the splat's kernel: a vertex is supported where some
  // sample's splat reaches its neighbourhood -- min_support = 1 and the component filters off.  Nobody has measured that these
  // are good values on real plots.  summary (may be NULL) receives finishMesh's.
  void create_mesh(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloud, pcl::PolygonMesh& mesh, sfmhip_mesh_finish_summary* summary = nullptr);
  // (ours) the similarity ICP that brings `cloud` onto `reference`, a cloud of the same scene in metres (a
  // terrestrial scan, last year's reconstruction, a surveyed subset): sfmhip_cloud_register with the scale estimated, from
  // `guess` (NULL: the identity; a large motion needs one).  Returns the metres per cloud unit that Dendrometry takes as
  // `scale` (also in *scale_out), 0 when the registration has too few pairs or is degenerate; `result` receives the whole
  // record.  max_dist: reference units, +inf keeps every pair.  Nothing calls it by default.
  double registerCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference, double* scale_out = nullptr,
                       double max_dist = INFINITY, const sfmhip_transform* guess = nullptr, sfmhip_register_result* result = nullptr);
  // (ours) the same through sfmhip_cloud_register_icp with the caller's options: the trimmed and one-to-one
  // rejectors, and with opts.metric 1 the point-to-plane metric against `reference_normals` (opts.normal_stride floats per
  // reference point; NULL: the reference's own k-NN normals, sfmhip_cloud_normals with k = 10, stride 4).  Returns
  // result->T.scale, 0 when a flag is set.
  double registerCloud(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference, const sfmhip_icp_opts& opts,
                       const float* reference_normals = nullptr, const sfmhip_transform* guess = nullptr, sfmhip_icp_result* result = nullptr);

  // (ours) the starting guess registerCloud needs when `cloud` and `reference` stand in unrelated gauges (two
  // reconstructions of one plot): each cloud is levelled by its own ground plane (sfmhip_cloud_ground_plane with `ground`, NULL:
  // the defaults), then sfmhip_cloud_align votes for scale, yaw and shift and runs ICP from every candidate.  `opts` needs
  // scale_lo, scale_hi and h_tol (sfmhip_align_default_opts sets the rest).  Returns the result's flags (0: result->reg.T is
  // the `guess` for registerCloud), or -1 when one of the clouds has no ground plane.  Nothing calls it by default.
  int alignPlots(pcl::PointCloud<pcl::PointXYZ>::Ptr& cloud, const pcl::PointCloud<pcl::PointXYZ>& reference, const sfmhip_align_opts& opts,
                 sfmhip_align_result* result, const sfmhip_ground_opts* ground = nullptr);

  const std::vector<cv::Mat>& colorImages() const { return mColorImages; }
  const std::vector<cv::Mat>& grayImages() const { return mGrayImages; }
  const std::vector<std::string>& imagePaths() const { return nImagesPath; }

  // ---- stand-ins for the out-of-scope front end: hand the pipeline state in directly
  void setDescriptors(const std::vector<cv::Mat>& d) {
    imagesDescriptors = d;
    releaseDeviceSet();
    releaseDeviceDescriptors();
    clearPairCache();
  }
  void setPoints2D(const std::vector<std::vector<cv::Point2d>>& p) { imagesPts2D = p; }
  void setCameraMatrix(const Intrinsics& k) { cameraMatrix = k; }
  void setCameraPoses(const std::vector<cv::Matx34d>& p) { nCameraPoses = p; }
  const std::vector<cv::Matx34d>& cameraPoses() const { return nCameraPoses; }
  const Intrinsics& intrinsics() const { return cameraMatrix; }
  void setMatchRatio(float r) { NN_MATCH_RATIO = r; }
  void setDoneViews(const std::set<int>& v) { nDoneViews = v; }
  void setGoodViews(const std::set<int>& v) { nGoodViews = v; }
  void clearPairCache() { pairCache.clear(); pairCacheOn = false; }
  // n images without pixels or descriptors: what the loops that count images (nImages, mGrayImages, imagesDescriptors) see
  void setImageCount(int n) {
    nImages.resize((size_t)n);
    mGrayImages.resize((size_t)n);
    if (imagesDescriptors.size() < (size_t)n) imagesDescriptors.resize((size_t)n);
  }
  // precomputed matches of pair (q, t), q < t: getMatching serves them from the pair cache
  void setPairMatches(int q, int t, const Matching& m) {
    pairCache[std::make_pair(q, t)] = m;
    pairCacheOn = true;
  }
  size_t pairCacheSize() const { return pairCache.size(); }
};
