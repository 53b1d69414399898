/*
 * sfmhip.h -- C ABI of the MI355X (gfx950) implementation of the feature-matching +
 * triangulation + bundle-adjustment hot path of codebydant/sfM_danPipeline.
 *
 * This is the drop-in boundary.  The reference has no plugin / FFI
 * layer: its boundary is three C++ member functions, which the host mirror in
 * sfm_danpipeline_amd/csrc/host/ (Sfm.h, BundleAdjustment.h) keeps verbatim and forwards here:
 *
 *   StructFromMotion::getMatching      reference include/Sfm.h:89,  src/Sfm.cpp:590-608
 *   StructFromMotion::triangulateViews reference include/Sfm.h:115-117, src/Sfm.cpp:804-878
 *   BundleAdjustment::adjustBundle     reference include/BundleAdjustment.h:19-20,
 *                                      src/BundleAdjustment.cpp:46-175
 *
 * Conventions: plain C types only; every function returns an int status (0 = ok, <0 = error,
 * see sfmhip_error_string); no exceptions cross this boundary; the caller owns every buffer
 * it passes; calls on one context are synchronous to the caller unless the name says
 * `_async`; a context is bound to one HIP device and is not thread-safe (the reference is
 * single-threaded, src/Sfm.cpp:9-109).  There is NO CPU fallback behind this ABI: without a
 * gfx950 device sfmhip_init fails.
 */
#ifndef SFMHIP_H
#define SFMHIP_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SFMHIP_VERSION 1

/* status codes */
enum {
  SFMHIP_OK = 0,
  SFMHIP_ERR_NO_DEVICE = -1,
  SFMHIP_ERR_HIP = -2,       /* a HIP runtime call failed; sfmhip_last_hip_error() has the code */
  SFMHIP_ERR_ARG = -3,
  SFMHIP_ERR_ALLOC = -4,
  SFMHIP_ERR_UNSUPPORTED = -5,
  SFMHIP_ERR_STATE = -6,
  SFMHIP_ERR_COMM = -7,
  SFMHIP_ERR_TIMEOUT = -8    /* a bounded spin inside a kernel ran out and the level-by-level fallback did too: a scheduling
                                fault or a bug, never a property of the data (a matrix that is not positive definite is an
                                invalid LM step, not an error) */
};

/* descriptor element type of a cv::Mat row (reference include/Sfm.h:29, src/Sfm.cpp:326) */
enum { SFMHIP_F32 = 0, SFMHIP_U8 = 1 };
/* distance.  L2 is what the reference always uses (cv::NORM_L2, src/Sfm.cpp:593) -- also on
 * binary ORB/AKAZE rows; HAMMING is cv::NORM_HAMMING as asked for by BASELINE.json cfg5. */
enum { SFMHIP_L2 = 0, SFMHIP_HAMMING = 1 };

typedef struct sfmhip_ctx sfmhip_ctx;
typedef struct sfmhip_imageset sfmhip_imageset;
typedef struct sfmhip_matchplan sfmhip_matchplan;
typedef struct sfmhip_ba sfmhip_ba;

/* ---- context ---- */
/* gfx950 devices visible to this process (>= 0), or a negative SFMHIP_ERR_*: what a one-process-per-GPU host program
 * maps its rank onto (device = local rank % count) */
int sfmhip_device_count(void);
int sfmhip_init(int device, sfmhip_ctx** out);
/* same, but all work is enqueued on an existing hipStream_t (e.g. torch's current stream) */
int sfmhip_init_on_stream(int device, void* hip_stream, sfmhip_ctx** out);
void sfmhip_shutdown(sfmhip_ctx* ctx);
int sfmhip_synchronize(sfmhip_ctx* ctx);
/* the context's HIP device and hipStream_t (for code that enqueues next to it: RCCL, see sfmhip_rccl.h) */
int sfmhip_device(sfmhip_ctx* ctx);
void* sfmhip_stream(sfmhip_ctx* ctx);
/* Stage timing (sfmhip_matchplan_last_timing, sfmhip_ba_last_timing) is opt-in: the hipEvents it
 * records between the stages of a run cost ~5-10 us of stream bubble each (3-4 % of a cfg2 sweep
 * or a cfg4 LM iteration).  Off by default; while off the *_last_timing calls report zeros. */
int sfmhip_set_timing(sfmhip_ctx* ctx, int enable);
/* Measurement probes (csrc/probe.hip; bench.py runs them on the box it benches, nothing on the product path calls them).
 * sfmhip_probe_i8_mfma_peak: what the chip sustains for bare v_mfma_i32_32x32x32_i8 on random operands, every SIMD busy, for
 * `seconds` (one launch): multiply-add operations per second (2 per MAC) and the shader clock that launch held -- the ceiling
 * to read the k-NN sweep's roofline fraction against, next to the nominal peak.  sfmhip_probe_clock_start / _read: a
 * one-wave kernel on THIS context's stream that watches the shader and the 100 MHz counters for `seconds` while the caller runs
 * the load to be qualified on another stream; _read waits for it and returns the shader clock in GHz.  Qualify the matcher
 * behind cv::BFMatcher::knnMatch, reference src/Sfm.cpp:593-599. */
int sfmhip_probe_i8_mfma_peak(sfmhip_ctx* ctx, double seconds, double* ops_per_s, double* shader_ghz);
int sfmhip_probe_clock_start(sfmhip_ctx* ctx, double seconds);
int sfmhip_probe_clock_read(sfmhip_ctx* ctx, double* shader_ghz);
const char* sfmhip_error_string(int status);
int sfmhip_last_hip_error(void);
int sfmhip_version(void);

/* ---- getMatching: one pair, host buffers (reference src/Sfm.cpp:590-608) ----
 * q,t: row-major descriptor matrices (nq x dim, nt x dim; dim = elements per row).
 * Emits, in ascending queryIdx, knn[i][0] of every query with d0 <= ratio*d1 (float compare),
 * k-NN ties broken towards the lower trainIdx exactly as cv::batchDistance does.
 * out_q/out_t/out_dist: caller-allocated, nq entries each.  nt < 2 emits nothing. */
int sfmhip_match_knn2(sfmhip_ctx* ctx, const void* q, int nq, const void* t, int nt, int dim,
                      int dtype, int norm, float ratio, int32_t* out_q, int32_t* out_t,
                      float* out_dist, int32_t* out_n);

/* ---- all-pairs matching with descriptors resident in HBM (the findBestPair loop,
 *      reference src/Sfm.cpp:511-515, as one batched launch) ---- */
int sfmhip_imageset_create(sfmhip_ctx* ctx, int n_images, const int32_t* n_rows, int dim,
                           int dtype, int norm, sfmhip_imageset** out);
/* copy one image's descriptor matrix host -> HBM */
int sfmhip_imageset_upload(sfmhip_imageset* set, int image, const void* host_rows);
/* or adopt rows that already live in HBM (no copy; must stay valid while the set is used) */
int sfmhip_imageset_adopt_device(sfmhip_imageset* set, int image, const void* device_rows);
/* device pass over every image: integrality check, centring to i8 / bit expansion, row norms,
 * tie-break key bases.  Asynchronous on the context's stream. */
int sfmhip_imageset_prepare_async(sfmhip_imageset* set);
void sfmhip_imageset_destroy(sfmhip_imageset* set);

/* pairs: n_pairs x (queryImage, trainImage) int32, host memory */
int sfmhip_matchplan_create(sfmhip_imageset* set, const int32_t* pairs, int n_pairs,
                            sfmhip_matchplan** out);
/* point an existing plan at another pair list (n_pairs <= the count it was created with): the
 * device buffers are reused, e.g. a one-pair plan serving every getMatching(q,t) call over a
 * resident image set (reference src/Sfm.cpp:426,977,1031) */
int sfmhip_matchplan_set_pairs(sfmhip_matchplan* plan, const int32_t* pairs, int n_pairs);
/* k-NN + ratio test + ordered compaction for every pair of the plan; results stay in HBM */
int sfmhip_matchplan_run_async(sfmhip_matchplan* plan, float ratio);
/* counts[n_pairs]; optional concatenated lists (capacity entries each, pair-major, ascending
 * queryIdx inside a pair); *total receives the number of matches over all pairs. */
int sfmhip_matchplan_fetch(sfmhip_matchplan* plan, int32_t* counts, int32_t* out_q,
                           int32_t* out_t, float* out_dist, int64_t capacity, int64_t* total);
/* Pipelined fetch -- what keeps getMatching's host-visible contract (a host Matching*, reference include/Sfm.h:89) from
 * costing a stall per sweep when sweeps follow each other (the all-pairs loop of findBestPair, src/Sfm.cpp:511-515, over
 * batches of pairs): once switched on, every sfmhip_matchplan_run_async is followed, on a second HIP stream, by a pass
 * that packs counts and {queryIdx | trainIdx | distance} lists straight into one of two pinned host buffers while the
 * first stream goes on with the next run.  capacity = matches a buffer holds (0: a quarter of n_pairs x max rows;
 * negative: switch the pipeline off again).
 * sfmhip_matchplan_fetch_wait(plan, back, ...) waits for the lists of the latest run (back = 0) or of the run before it
 * (back = 1) and hands out pointers INTO the pinned buffer: counts[n_pairs], then total entries each of q, t, dist,
 * pair-major -- valid until two more runs have been enqueued.  SFMHIP_ERR_ALLOC with *total set when a run found more
 * matches than a buffer holds (switch the pipeline on again with that capacity; sfmhip_matchplan_fetch still works). */
int sfmhip_matchplan_pipeline(sfmhip_matchplan* plan, int64_t capacity);
int sfmhip_matchplan_fetch_wait(sfmhip_matchplan* plan, int back, const int32_t** counts, const int32_t** out_q,
                                const int32_t** out_t, const float** out_dist, int64_t* total);
/* raw k=2 lists of pair `pair`: idx[nq*2] (-1 padded), dist[nq*2] */
int sfmhip_matchplan_fetch_knn(sfmhip_matchplan* plan, int pair, int32_t* idx, float* dist);
/* seconds of device time of the last run's kernels, by stage (hipEvents on the ctx stream):
 * [0]=prepare (last prepare_async) [1]=knn kernels [2]=compaction; and the knn-kernel count */
int sfmhip_matchplan_last_timing(sfmhip_matchplan* plan, double seconds[3]);
/* seconds of the last run's k-NN kernel alone -- the one launch the MFMA roofline is priced on (stage [1]
 * above also holds the exact / fix-up kernels that follow it) */
int sfmhip_matchplan_last_knn_kernel_time(sfmhip_matchplan* plan, double* seconds);
void sfmhip_matchplan_destroy(sfmhip_matchplan* plan);

/* ---- triangulateViews numerics (reference src/Sfm.cpp:812-860) ----
 * P1,P2: cv::Matx34d row-major; K 3x3 row-major; dist k1,k2,p1,p2,k3; xy1/xy2: m gathered
 * pixel pairs (AlignedPoints, src/Sfm.cpp:694-711).  X: 3*m, keep: m (1 = both reprojection
 * errors <= max_err as float), err: 2*m floats or NULL.  The test is the reference's
 * !(max_err < e1 || max_err < e2): a row whose error is NaN (a non-finite observation, say) is
 * KEPT, with its NaN point, as in the reference; so is every row under a NaN max_err. */
int sfmhip_triangulate(sfmhip_ctx* ctx, const double P1[12], const double P2[12],
                       const double K[9], const double dist[5], const double* xy1,
                       const double* xy2, int m, float max_err, double* X, float* err,
                       uint8_t* keep);

/* ---- incremental-loop glue next to the hot path ----
 * find2D3DMatches, the 2D-3D association (reference src/Sfm.cpp:1047-1090).  The cloud's tracks
 * (Point3D::idxImage, a std::map ordered by view) come as CSR: entries trk_ptr[p]..trk_ptr[p+1]-1
 * of (trk_view, trk_feat), ascending view.  For every cloud point, in cloud order: its feature
 * in done_view, then the FIRST match (match order) whose queryIdx (done_view < new_view) or
 * trainIdx (otherwise) is that feature; emits (cloud index, feature index in the new view).
 * As in the reference's loop (matched2DPointInNewView starts at -1 and the scan only stops at a
 * value >= 0, src/Sfm.cpp:1062-1082), a match whose other-side index is negative is passed over:
 * FIRST means the first match on the key whose other side is >= 0.  A point with no such match,
 * no entry in done_view, or a feature that no match keys, emits nothing.  Feature indices are
 * indices: a negative track feature or key-side index never matches anything (the reference's
 * == would pair two equal negative values; getMatching produces none).
 * out_cloud/out_feat: n_cloud entries each. */
int sfmhip_find_2d3d(sfmhip_ctx* ctx, const int32_t* trk_ptr, const int32_t* trk_view,
                     const int32_t* trk_feat, int n_cloud, int done_view, int new_view,
                     const int32_t* match_q, const int32_t* match_t, int n_match,
                     int32_t* out_cloud, int32_t* out_feat, int32_t* n_out);
/* mergeNewPoints (reference src/Sfm.cpp:1212-1244): new point i is appended iff no point
 * already in the cloud -- the existing ones and the new points appended before it -- lies closer
 * than min_dist (cv::norm of the difference in double, against the float literal promoted to
 * double).  accept: n_new bytes (1 = appended). */
int sfmhip_merge_new_points(sfmhip_ctx* ctx, const double* cloud_xyz, int n_cloud,
                            const double* new_xyz, int n_new, float min_dist, uint8_t* accept,
                            int32_t* n_accepted);

/* ---- the detector / descriptor front end of getFeature (reference src/Sfm.cpp:300-330) ----
 * cv::xfeatures2d::SIFT::create(nfeatures = 0, nOctaveLayers, contrastThreshold, edgeThreshold, sigma)
 *     ->detectAndCompute(gray, noArray(), keypoints, descriptors)
 * as OpenCV 3.4.1's float pipeline computes it (doubled base image, Gaussian / DoG pyramids, refined extrema,
 * orientation peaks, removeDuplicatedSorted, 4x4x8 descriptors x512 saturated to 8 bit and stored as float).
 * gray: rows x cols 8-bit, host memory.  keypoints: 6 floats each -- pt.x, pt.y, size, angle, response, and the
 * int32 `octave` field bit-copied into the sixth float -- in OpenCV's sorted order; descriptors: 128 floats each
 * (integer values 0..255: the input layout of the matcher).  capacity: keypoints the output arrays hold; 0 with null
 * arrays = count only.  *n_keypoints receives the count; more than `capacity` returns SFMHIP_ERR_ARG.
 * Parity unpinned (OpenCV is not available here): see DESIGN.md section 1, row f-3. */
int sfmhip_sift_detect_and_compute(sfmhip_ctx* ctx, const uint8_t* gray, int rows, int cols, int n_octave_layers,
                                   double contrast_threshold, double edge_threshold, double sigma, int capacity,
                                   float* keypoints, float* descriptors, int32_t* n_keypoints);
/* The same with the descriptors LEFT IN HBM: *d_descriptors receives a device array of n_keypoints x 128 f32 rows that
 * the caller owns (sfmhip_device_free) and can hand to sfmhip_imageset_adopt_device -- the reference keeps keypoints and
 * descriptors of an image in one container (src/Sfm.cpp:326) and matches them right away; here the rows never leave the
 * device between extraction and matching.  keypoints: host, capacity x 6 floats as above (capacity 0: count only). */
int sfmhip_sift_detect_and_compute_device(sfmhip_ctx* ctx, const uint8_t* gray, int rows, int cols, int n_octave_layers,
                                          double contrast_threshold, double edge_threshold, double sigma, int capacity,
                                          float* keypoints, void** d_descriptors, int32_t* n_keypoints);
/* extractFeature's loop (reference src/Sfm.cpp:283-290) as one call: n_images gray images, several in flight on worker
 * streams of the context (an image's front end is ~100 small launches and two read-backs: latency the next image hides).
 * keypoints[i]: a host array of n_keypoints[i] x 6 floats allocated by the library (sfmhip_host_free); d_descriptors[i]: a
 * device array of n_keypoints[i] x 128 f32 (sfmhip_device_free).  Image by image the results of the one-image entry.
 * An image the one-image entry would refuse (null, a side below 2) refuses the whole call with SFMHIP_ERR_ARG before
 * any output is written; n_images = 0 is SFMHIP_OK. */
int sfmhip_sift_batch(sfmhip_ctx* ctx, int n_images, const uint8_t* const* gray, const int32_t* rows, const int32_t* cols,
                      int n_octave_layers, double contrast_threshold, double edge_threshold, double sigma, float** keypoints,
                      void** d_descriptors, int32_t* n_keypoints);
void sfmhip_device_free(void* device_ptr);
void sfmhip_host_free(void* host_ptr);
/* device -> host copy of bytes the library left in HBM (e.g. descriptor rows), on the context's stream, synchronous */
int sfmhip_device_download(sfmhip_ctx* ctx, void* host_dst, const void* device_src, size_t bytes);

/* ---- the scoring half of findBestPair (reference src/Sfm.cpp:536-563) ----
 * For every pair of a batch the inlier count of
 *   cv::findEssentialMat(alignedLeft, alignedRight, K, CV_RANSAC, prob, threshold, mask)       (src/Sfm.cpp:542-543)
 * as OpenCV 3.4.1 computes it: points normalised as p * (1 / f) + (-c / f), threshold / ((fx + fy) / 2), cv::RNG
 * restarted at (uint64)-1, five distinct sample indices, the models of a sample in turn, goodCount > max(best, 4)
 * updates the best and the iteration limit (RANSACUpdateNumIters, at most 1000), error = squared epipolar residual
 * over the four squared line coefficients as a float <= (float)(t*t).  The five-point solver follows the library's
 * runKernel step by step (Jacobi-SVD null space, 10 x 20 elimination, tenth-degree polynomial, solvePoly's
 * Durand-Kerner iteration, real iff |imag| <= 1e-10, SVD::solveZ, models in root order); OpenCV is not available to
 * pin it against.
 * offsets: n_pairs + 1 prefix sums of the match counts; left_xy / right_xy: 2 doubles per match (pixels), pair after
 * pair (host memory); inliers: n_pairs; mask (optional): one byte per match; iterations (optional): RANSAC iterations
 * run per pair.  Pairs with fewer than 5 matches score 0 (findEssentialMat returns an empty matrix). */
int sfmhip_score_essential(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                           const double* right_xy, double fx, double fy, double cx, double cy, double prob,
                           double threshold, int32_t* inliers, uint8_t* mask, int32_t* iterations);

/* OR over the five-point samples of the context's last sfmhip_score_essential call: bit 0 = two Durand-Kerner
 * iterates coincided bit for bit, bit 1 = the polynomial's leading coefficient was <= DBL_EPSILON -- the two corners
 * of cv::solvePoly whose library behaviour (a cube-root branch; part of a work buffer returned as roots) is not
 * reproduced.  0 = every sample went the documented way. */
int sfmhip_score_last_flags(sfmhip_ctx* ctx);
/* EMEstimatorCallback::runKernel (OpenCV 3.4.1 calib3d/five-point.cpp) for explicit samples: q1 / q2 = n_samples x five
 * normalised points (x, y) each; models: n_samples x 10 row-major 3 x 3 matrices (unit Frobenius norm, the library's
 * order: the order of solvePoly's roots); n_models[i] = count | flags << 8 (flags as sfmhip_score_last_flags).  What the
 * RANSAC above runs per iteration, exposed for sample-level parity checks. */
int sfmhip_score_five_point(sfmhip_ctx* ctx, int n_samples, const double* q1, const double* q2, double* models,
                            int32_t* n_models);

/* The homography side of the same loop: findHomographyInliers (reference src/Sfm.cpp:667-689) =
 *   cv::countNonZero(mask) of cv::findHomography(query_points, train_points, CV_RANSAC, 0.004 * maxVal, mask)
 * as OpenCV 3.4.1 (calib3d/fundam.cpp) runs it: points converted to float, 4-point samples (drawn again when
 * checkSubset rejects them: a collinear triple, or the orientation of a triple not preserved), normalised DLT
 * (smallest eigenvector of L^T L, H[2][2] = 1), the reprojection error and the threshold test in float arithmetic,
 * confidence / max_iters as given (findHomography's defaults: 0.995, 2000); the mask is the RANSAC mask.
 * thresholds: one per pair (the reference: 0.004 * the largest coordinate among the pair's query points; <= 0: 3).
 * Pairs with fewer than 4 matches score 0.  Parity unpinned, like sfmhip_score_essential. */
/* HomographyEstimatorCallback::runKernel (OpenCV 3.4.1 calib3d/fundam.cpp) for explicit samples: M / m = n_samples x four
 * float points (x, y); H: n_samples x 9 doubles (scaled by 1 / H[8], as the library does); ok[i] = 0 for a degenerate sample.  For sample-level parity checks. */
int sfmhip_score_homography_kernel(sfmhip_ctx* ctx, int n_samples, const float* M, const float* m, double* H, int32_t* ok);
int sfmhip_score_homography(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                            const double* right_xy, const double* thresholds, double confidence, int max_iters,
                            int32_t* inliers, uint8_t* mask, int32_t* iterations);

/* ---- the pose step of baseReconstruction: getCameraPose (reference src/Sfm.cpp:713-789) ----
 * cv::recoverPose(E, p1, p2, R, t, focal, pp, mask) as OpenCV 3.4.1 (calib3d/five-point.cpp) runs it, with
 * K = [f 0 ppx; 0 f ppy; 0 0 1] (the focal / principal-point overload: ONE focal for both axes):
 *   1. x' = x * (1 / f) + (-ppx * (1 / f)), y' likewise with ppy and the same f (findEssentialMat's MatExpr route);
 *   2. decomposeEssentialMat(E): SVD::compute (JacobiSVDImpl_<double> on E^T: the rotation rule, convergence test,
 *      descending selection sort and 1 / sd scaling of U of the five-point and triangulation code), U and Vt negated
 *      when their determinant is negative, W = [0 1 0; -1 0 0; 0 0 1], R1 = U W Vt, R2 = U W^T Vt, t = U.col(2).  A
 *      singular value <= DBL_MIN sends the library to a random-vector branch (RNG(0x12345678)) that is NOT restated:
 *      sfmhip_pose_last_flags reports it (bit 0) and that column of U is left zero;
 *   3. per candidate P1 = [R1|t], P2 = [R2|t], P3 = [R1|-t], P4 = [R2|-t] and per point: Q = triangulatePoints([I|0], Pi,
 *      x1', x2') (the 4 x 4 DLT of sfmhip_triangulate), ok = Q2 Q3 > 0, Q /= Q3 (row 3: Q3 / Q3), ok &= Q2 < dist,
 *      z = Pi.row(2) Q summed in k order, ok &= z > 0 && z < dist (a comparison with a NaN is false);
 *   4. mask_in (nullable) ANDed into all four masks (bitwise_and: the output byte is the input byte where the chosen
 *      candidate passes, 255 where it passes without an input mask, 0 elsewhere);
 *   5. good_i = countNonZero(mask_i); the first of good1, good2, good3 that is >= every other count picks (R1, t),
 *      (R2, t), (R1, -t), else (R2, -t); n_good = its count, mask_out = its mask.
 * distance_thresh: the library's default is 50.  Offsets / points as sfmhip_score_essential; E: 9 doubles per pair,
 * row-major; R: 9 per pair, t: 3 per pair.  Parity UNPINNED like the score entries (OpenCV is not in the image). */
int sfmhip_recover_pose(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                        const double* right_xy, const double* E, double focal, double ppx, double ppy,
                        double distance_thresh, const uint8_t* mask_in /* nullable */, double* R /* 9/pair */,
                        double* t /* 3/pair */, int32_t* n_good, uint8_t* mask_out /* nullable */);
/* getCameraPose's numerics for a batch: findEssentialMat(K, RANSAC, prob, threshold) exactly as sfmhip_score_essential
 * (same inliers, same mask), then recoverPose(E, ..., fx, (cx, cy), mask) with the RANSAC mask as input and
 * distance_thresh 50, E never leaving the device.  fy serves the RANSAC's normalisation only.  Pairs without a model
 * (fewer than five matches, or no sample gave one): inliers 0, n_good -1, E / R / t zero, mask zero.  A pair of exactly
 * five matches poses with the first model of its one sample.  CheckCoherentRotation is the caller's. */
int sfmhip_essential_pose(sfmhip_ctx* ctx, int n_pairs, const int32_t* offsets, const double* left_xy,
                          const double* right_xy, double fx, double fy, double cx, double cy, double prob,
                          double threshold, double* E, int32_t* inliers, double* R, double* t, int32_t* n_good,
                          uint8_t* mask /* nullable: recoverPose's output mask */);
/* OR over the decompositions of the last sfmhip_recover_pose / sfmhip_essential_pose call: bit 0 = a singular value of
 * E was <= DBL_MIN (OpenCV's random-vector branch, not restated).  0 = every pair went the documented way. */
int sfmhip_pose_last_flags(sfmhip_ctx* ctx);

/* ---- camera registration: findCameraPosePNP (reference src/Sfm.cpp:1137-1210) ----
 * cv::solvePnPRansac(pts3D, pts2D, K, dist, rvec, T, useExtrinsicGuess, max_iters, threshold, confidence, inliers, CV_EPNP)
 * for a batch of views.  THE CONTRACT IS THE RULE LIST BELOW, not "what OpenCV does": OpenCV is not in the image, so
 * parity is UNPINNED; the rules are written as 3.4.1 (calib3d/solvepnp.cpp, epnp.cpp, ptsetreg.cpp) is understood to run
 * them, and a rule marked † is a reading from memory that nothing here can check.
 *  RANSAC shape
 *   1. object and image points are converted to float32 first †; a view of fewer than 5 correspondences has status -1
 *      (exactly 4, the library's P3P branch, is not built and reports -1 too);
 *   2. 5 model points; cv::RNG restarts at (uint64)-1 in every call, so a view's samples depend on its correspondence count
 *      alone; the subset draw is getSubset's (an index drawn before is drawn again); the default checkSubset accepts every
 *      sample; a view of exactly 5 correspondences is its one sample, every point an inlier, 0 iterations;
 *  one model per sample
 *   3. undistortPoints (five fixed-point iterations) on the 5 float pixels, its output stored as float32 †, then EPnP
 *      with an identity camera matrix † on the float points read as f64:
 *      control points = centroid + sqrt(d_i / n) * principal axis i of the 3 x 3 covariance (cvSVD, U^T rows);
 *      barycentric alphas through cvInvert(CC, CV_SVD) (SVD::backSubst: singular values <= 2 eps sum(w) skipped);
 *      M (2n x 12), M^T M, its SVD by the library's one-sided Jacobi (JacobiSVDImpl_<double>, glibc's hypot), rows
 *      11, 10, 9, 8 of U^T as the four smallest eigenvectors; L_6x10 and rho; betas for N = 1, 2, 3 by cvSolve(CV_SVD);
 *      five Gauss-Newton steps each with the file's own Householder QR (its column maximum looks at rows k .. nr - 2 †);
 *      R and t from the 3 x 3 SVD of the Procrustes sum with the determinant fix, after solve_for_sign by the first
 *      point's depth; the N with the smallest mean reprojection error wins (ties: the smaller N); Rodrigues(R) = rvec;
 *   4. NOT the library's: (a) every sum over the points of a problem is taken in one fixed order (slot i mod 256, each 64
 *      slots folded by strides 32..1, the four groups as (g0 + g1) + (g2 + g3)), so that one thread, one workgroup and the
 *      CPU build give the same bits; (b) sin, cos and acos in Rodrigues are plain-f64 restatements (measured: at most 1 ulp from libm; the test allows 2), not
 *      libm's; (c) a point set whose covariance has a third singular value <= 1e-12 of its first (planar, collinear) is
 *      not solved: the hypothesis is skipped and bit 0 of sfmhip_pnp_last_flags is set;
 *  error and inliers
 *   5. projectPoints(float point, Rodrigues(rvec), tvec, K, dist) in f64, stored as float32; err = dx * dx + dy * dy in
 *      float; inlier iff err <= (float)(thr * thr);
 *  best model and stopping
 *   6. a model replaces the best when its count > max(best, 4); the limit becomes RANSACUpdateNumIters(confidence,
 *      (n - count) / n, 5, limit) with the host's libm; status 0 when no model ever did;
 *  refit and the returned pose
 *   7. on success EPnP runs once more on all inliers (the float points back as f64, undistortPoints in f64);
 *   8. which pose 3.4.1 returns †: the RANSAC model; the refit only decides success (EPnP always succeeds).  rvec / tvec
 *      follow that reading; rvec_ransac / tvec_ransac and rvec_refit / tvec_refit hand out both.
 *  options and edges
 *   9. max_iters == 0: no sample is drawn; a view of more than 5 correspondences has status 0, 0 inliers, 0 iterations and
 *      zero outputs (a view of exactly 5 is still its one sample).  max_iters < 0 is refused.  `iterations` counts the
 *      samples tried, skipped ones included, so it never exceeds max_iters;
 *  10. confidence is clamped to [0, 1] inside RANSACUpdateNumIters: at or below 0 the limit drops to 0 with the first model
 *      that has more than 4 inliers, and the loop ends there; at or above 1 the limit never drops and the loop runs
 *      max_iters iterations.  Nothing is refused;
 *  11. a threshold of 0 accepts exact reprojections only (in practice: no model, max_iters iterations); thr * thr is taken
 *      to float32, so a threshold above 1.8e19 px is infinite and accepts every error that is not NaN;
 *  12. non-finite input: the call returns (every loop of a solve has a fixed trip count).  A sample that holds a NaN or
 *      an Inf object coordinate fails rule 4c's test, is skipped and sets bits 0 and 1 of sfmhip_pnp_last_flags; one that
 *      holds a non-finite pixel sets bit 1 and gives a model with NaN entries, which has no inlier.  A correspondence with a non-finite
 *      coordinate has a NaN error and is never an inlier, so it is outside the mask and the refit; a view of nothing
 *      else has status 0 after max_iters iterations.  Other views are not affected;
 *  13. Rodrigues(R) within 1e-5 of a half turn (|axis part| / 2 < 1e-5, trace < 1) takes the library's diagonal formula:
 *      rx >= 0, so the vector may describe the turn's other sense (up to twice the angle's distance from pi away), and
 *      an error d in a diagonal entry near -1 moves the rotation by up to 2 sqrt(d); within 1e-5 of the identity the
 *      vector is exactly zero; a matrix with an entry outside [-100, 100) or NaN gives the zero vector.
 * SFMHIP_ERR_ARG, with nothing written: ctx, offsets, K, dist, thresholds, status, rvec, tvec or inliers NULL; n_views < 0;
 * max_iters < 0; offsets[0] != 0 or decreasing offsets; xyz or xy NULL with offsets[n_views] > 0.  n_views == 0 is
 * SFMHIP_OK and writes nothing.
 * offsets: n_views + 1, offsets[0] = 0; xyz: 3 doubles, xy: 2 doubles (pixels) per correspondence; thresholds: pixels, one
 * per view; status / inliers / iterations: per view; rvec / tvec (and the nullable _ransac, _refit pairs): 3 doubles per
 * view, zero without a model; mask (nullable): 1 byte per correspondence, the best model's inliers.  Views are
 * independent of each other. */
int sfmhip_pnp_ransac(sfmhip_ctx* ctx, int n_views, const int32_t* offsets, const double* xyz, const double* xy,
                      const double K[9], const double dist[5], const double* thresholds, double confidence,
                      int max_iters, int32_t* status, double* rvec, double* tvec, double* rvec_ransac /* nullable */,
                      double* tvec_ransac /* nullable */, double* rvec_refit /* nullable */,
                      double* tvec_refit /* nullable */, int32_t* inliers, uint8_t* mask /* nullable */,
                      int32_t* iterations /* nullable */);
/* The EPnP solve of rule 3 alone for explicit point sets of any size >= 5 (xy_normalised: 2 doubles per point, already
 * undistorted and normalised): R 9 doubles (row-major), t 3 doubles per problem, zero for a set rule 4c refuses.  What
 * the RANSAC runs per sample and the refit per view, exposed for sample-level checks.  SFMHIP_ERR_ARG, with nothing
 * written: ctx, offsets, R or t NULL; n_problems < 0; offsets[0] != 0 or decreasing offsets; xyz or xy_normalised NULL; a
 * problem of fewer than 5 points.  n_problems == 0 is SFMHIP_OK and writes nothing. */
int sfmhip_pnp_epnp(sfmhip_ctx* ctx, int n_problems, const int32_t* offsets, const double* xyz,
                    const double* xy_normalised, double* R, double* t);
/* OR over the solves of the last sfmhip_pnp_ransac / sfmhip_pnp_epnp call: bit 0 = a rank-deficient control-point
 * covariance (rule 4c), bit 1 = a 3 x 3 singular value <= DBL_MIN (the library's random-vector branch, not restated),
 * bit 2 = qr_solve met a zero column (the library then uses an uninitialised step; here the step is 0).  0 = every solve
 * went the documented way. */
int sfmhip_pnp_last_flags(sfmhip_ctx* ctx);
/* With sfmhip_set_timing on: the kernel time (ms, by events on the context's stream) of the last sfmhip_pnp_ransac call:
 * ms3 = solver, scoring, mask + refit. */
int sfmhip_pnp_last_timing(sfmhip_ctx* ctx, double* ms3);

/* ---- map3D step 10: the dense cloud's filters and normals (reference src/Sfm.cpp:94-102, bodies :1323-1383) ----
 * PCL 1.8.1's PassThrough, RadiusOutlierRemoval and NormalEstimation (k nearest) on a device-resident cloud: the points
 * are uploaded once by sfmhip_cloud_create and every call below reuses them and the spatial grid built for them (one
 * grid per radius last used, one k-NN grid).  The rules (parity UNPINNED, PCL is not in the image):
 *   - a point with a non-finite coordinate is dropped by both filters, is nobody's neighbour, and has -1 / +inf k-NN
 *     entries and a NaN normal and curvature;
 *   - d2 = ((dx*dx) + dy*dy) + dz*dz in float (FLANN L2_Simple); the radius test is d2 < (float)(r * r), r squared in
 *     double; the count includes the point itself and its duplicates;
 *   - k-NN lists are sorted by (d2, index) and include the point itself; k > the finite count pads with -1 / +inf;
 *   - normals: PCL's float covariance of the k nearest (9 sums in list order, divided by the count), pcl::eigen33 (its
 *     trigonometric roots, with atan2 / cos / sin restated from + - * / sqrt), curvature |lambda0 / trace| (0 for a zero
 *     trace), then flipped iff (vp - p) . n < 0; fewer than 3 neighbours: NaN.  Every NaN written is 0x7FC00000.
 * Index outputs are input indices in input order; idx_out holds up to n entries.  A handle belongs to its context and
 * is not thread-safe; several handles may live on one context. */
typedef struct sfmhip_cloud sfmhip_cloud;
int sfmhip_cloud_create(sfmhip_ctx* ctx, int n, const float* xyz /* 3 n */, sfmhip_cloud** out);
void sfmhip_cloud_destroy(sfmhip_cloud* cloud);
/* PassThrough on field `axis` (0 x, 1 y, 2 z) with float limits, inclusive: kept iff lo <= v <= hi (negative != 0: iff
 * not); non-finite points are never kept.  *n_out = the kept count. */
int sfmhip_cloud_passthrough(sfmhip_cloud* cloud, int axis, float lo, float hi, int negative, int32_t* idx_out,
                             int32_t* n_out);
/* per point: the number of finite points with d2 < (float)(radius * radius), itself included; cap > 0 reports
 * min(count, cap) (and lets the kernel stop early), cap <= 0 the exact count.  Non-finite points: 0. */
int sfmhip_cloud_radius_count(sfmhip_cloud* cloud, double radius, int cap, int32_t* counts /* n */);
/* RadiusOutlierRemoval: kept iff the count above is > min_pts (a count <= min_pts is an outlier). */
int sfmhip_cloud_radius_outlier(sfmhip_cloud* cloud, double radius, int min_pts, int32_t* idx_out, int32_t* n_out);
/* the k (1..32) nearest finite points of every point, (d2, index) order: idx / d2 are n x k, row-major. */
int sfmhip_cloud_knn(sfmhip_cloud* cloud, int k, int32_t* idx, float* d2);
/* NormalEstimation with setKSearch(k), k in 1..32, viewpoint vp[3]: out4 = n x (nx, ny, nz, curvature). */
int sfmhip_cloud_normals(sfmhip_cloud* cloud, int k, const float* vp /* 3 */, float* out4);

/* ---- thinning and noise removal on the same cloud: PCL 1.8.1's VoxelGrid and StatisticalOutlierRemoval ----
 * The reference calls neither; the rules are PCL's as recalled (parity UNPINNED, PCL is not in the image; + marks what
 * is ours).  csrc/cloud_filter.h holds them as code.
 *   V1. leaf[3]: floats, each > 0 and finite (else SFMHIP_ERR_ARG); inv[a] = 1.0f / leaf[a] in float.
 *   V2. min_p / max_p: the box of the finite points as floats.  d[a] = (int64)((max_p[a] - min_p[a]) * inv[a]) + 1 in float
 *       arithmetic with a truncating cast; d[0] d[1] d[2] > INT32_MAX: SFMHIP_ERR_UNSUPPORTED, nothing written (PCL warns
 *       and copies the input).  + The same refusal when floor(min_p[a] * inv[a]) or floor(max_p[a] * inv[a]) does not fit
 *       an int32, when the product of the actual extents div[a] = max_b[a] - min_b[a] + 1 exceeds INT32_MAX, and when one
 *       div[a] exceeds 2^24 (the float difference of V3 would no longer be exact).
 *   V3. min_b[a] = (int)floor(min_p[a] * inv[a]); ijk[a] = (int)(floor(p[a] * inv[a]) - (float)min_b[a]), all in float;
 *       idx = ijk[0] + ijk[1] div[0] + ijk[2] div[0] div[1].  A non-finite point is in no voxel.
 *   V4. a voxel is emitted iff it holds at least min_points (>= 0) points; the output is in ascending idx.
 *   V5. centroid: float sums of x, y and z, then sum / (float)count per component.  + The order: the voxel's points in
 *       ascending input index, cut into consecutive blocks of 64; each block summed sequentially from 0.0f, the block
 *       sums added sequentially in ascending order from 0.0f (a voxel of at most 64 points: one sequential sum).
 *   V6. rgb (0x00RRGGBB per point): u64 channel sums, truncating integer division, top byte 0 -- PCL's float accumulate
 *       and uint8 cast while a channel sum stays below 2^24.  normals (3 floats per point): summed by V5's order, then
 *       each component divided by sqrt((x*x + y*y) + z*z) in float; a length of zero or NaN gives 0x7FC00000 in all three,
 *       so a NaN input normal propagates.
 *   V7. voxel_of[i]: the output row of point i's voxel, -1 for a non-finite point or a voxel V4 dropped.
 *   S1. mean_k in 1..63; every finite point's mean_k + 1 nearest finite points by the d2 above, itself and its
 *       duplicates included, in ascending d2.
 *   S2. dist_sum = sum over k = 1..mean_k of sqrt((double)d2[k]), sequential in ascending k, in f64; mean_dist =
 *       (float)(dist_sum / mean_k); 0 for a non-finite point, which is never kept.
 *   S3. sum += (double)md, sq += (double)(md * md) (float product).  + The order: consecutive blocks of 256 input
 *       indices, each summed sequentially from 0.0, the partials added sequentially in ascending order.  mean = sum / N,
 *       var = (sq - sum * sum / N) / (N - 1) over the N finite points, + clamped to 0 from below; thr = mean + std_mul sqrt(var).
 *   S4. kept iff (double)md <= thr; negative != 0: iff (double)md > thr.
 *   S5. no finite point: SFMHIP_OK, nothing kept, threshold 0.  0 < N <= mean_k: SFMHIP_ERR_ARG, nothing written (PCL
 *       reads stale list slots there).  std_mul must be finite. */
/* rgb / normals: n / 3 n values or NULL.  out_xyz / out_rgb / out_normals: room for n / n / 3 n values, each may be NULL
 * (an attribute without its input is not written).  voxel_of: n or NULL.  out_cloud: NULL, or it receives a new handle on
 * the same context whose points are the centroids -- they are on the device already and are not uploaded again. */
int sfmhip_cloud_voxel_grid(sfmhip_cloud* cloud, const float leaf[3], int min_points, const uint32_t* rgb, const float* normals,
                            float* out_xyz, uint32_t* out_rgb, float* out_normals, int32_t* voxel_of, int32_t* n_out,
                            sfmhip_cloud** out_cloud);
/* idx_out: the kept input indices in input order (room for n); mean_dist: n or NULL; threshold: thr or NULL */
int sfmhip_cloud_statistical_outlier(sfmhip_cloud* cloud, int mean_k, double std_mul, int negative, int32_t* idx_out,
                                     int32_t* n_out, float* mean_dist, double* threshold);
/* a new handle over the points indices[0..n_idx) of this one, gathered on the device: duplicates allowed, order kept;
 * an index outside [0, n) is SFMHIP_ERR_ARG */
int sfmhip_cloud_select(sfmhip_cloud* cloud, const int32_t* indices, int n_idx, sfmhip_cloud** out);
/* the point count and the count of finite points (either may be NULL) */
int sfmhip_cloud_size(const sfmhip_cloud* cloud, int32_t* n, int32_t* n_valid);
/* the handle's points (what a handle born on the device holds) */
int sfmhip_cloud_download(sfmhip_cloud* cloud, float* xyz /* 3 n */);
/* With sfmhip_set_timing on (zeros while it is off): host-clock ms of the last voxel grid call on this handle -- key +
 * sort, voxel reduce -- and of its last outlier call -- neighbour means, threshold + compaction. */
int sfmhip_cloud_filter_last_timing(sfmhip_cloud* cloud, double ms4[4]);

/* ---- smoothing on the same cloud: PCL 1.8.1's MovingLeastSquares ----
 * computeMLSPointNormal with no upsampling (NONE) and SIMPLE projection: every point is moved onto the plane, or the
 * polynomial surface, fitted to its neighbours within search_radius.  The reference's create_mesh still carries the remains
 * of this pass (src/Sfm.cpp:1347-1383) but does not call it.  The rules are PCL's as recalled (parity UNPINNED, PCL is not
 * in the image).  This list is the contract; csrc/mls.h holds it as code.  A dagger marks what nothing here can check, + what
 * is ours.
 *   M1. neighbours of point i: the finite points with d2 < (float)(r * r), d2 = ((dx dx) + dy dy) + dz dz in float (the
 *       radius search of sfmhip_cloud_radius_count), i itself and its duplicates included.  A non-finite point is nobody's
 *       neighbour and is not output.
 *   M2. + order: every sum over a point's neighbours runs sequentially from zero in ascending (cell key, input index).  The
 *       key is that of the radius grid for r: origin = the box minimum of the finite points; cell = r (1 + 2^-10), doubled
 *       while prod_a min(floor(extent_a / cell) + 1, 2^12) exceeds 2^22; a coordinate's cell = floor((v - origin) / cell) in
 *       double, clamped to [0, D_a - 1]; key = (cz D_y + cy) D_x + cx.  The result is a function of the points and the
 *       options alone.
 *   M3. (dagger) fewer than 3 neighbours: the point is dropped.  Otherwise, in double: the nine sums xx xy xz yy yz zz x y z,
 *       each divided by the count, cov = E[ab] - E[a]E[b]; pcl::eigen33 (scale by the largest |entry|, 1 when that is <=
 *       DBL_MIN; the trigonometric roots, the quadratic when |c0| < DBL_EPSILON or the smallest root is <= 0; the largest
 *       of the three row cross products of cov / scale - root0 I, normalised) gives the plane normal n and lambda0; d = -n.mean,
 *       dist = p.n + d, q = p - dist n, curvature = |lambda0 / trace| (0 for a zero trace).  Dots are (a0 b0 + a1 b1) + a2 b2.
 *   M4. + n not finite (all neighbours identical or exactly collinear): the point is output unmoved, its normal and curvature
 *       are NaN (0x7FC00000), and it is counted in n_degenerate.
 *   M5. (dagger) polynomial_order 0 (PCL's setPolynomialFit(false)) stops at M3.  Order 1 has 3 coefficients, order 2 has 6; with
 *       fewer neighbours than coefficients M3's result stands (n_plane_only).  Otherwise per neighbour x: e = x - q, w =
 *       exp(-(e.e) / g) with g = sqr_gauss_param, or r r in double when that is <= 0; v_axis = Eigen's unitOrthogonal of n
 *       ((-ny, nx, 0) / sqrt(nx nx + ny ny) unless |nx| and |ny| are both <= 1e-12 |nz|, then (0, -nz, ny) / sqrt(ny ny +
 *       nz nz)), u_axis = n x v_axis; u = e.u_axis, v = e.v_axis, f = e.n; terms t = u^a v^b for a = 0..order, b =
 *       0..order - a, powers by repeated multiplication.  A = sum w (u^a v^b) over the distinct exponent pairs and b = sum
 *       (w t) f by M2's order; Cholesky (LLT), forward then back substitution, each inner sum subtracted in ascending index;
 *       q += c[0] n, normal = n - c[order + 1] u_axis - c[1] v_axis, normalised.  The curvature stays M3's.  + A pivot that is
 *       <= 0 or not finite, or a coefficient that is not finite, keeps M3's result (n_fit_failed).
 *   M6. + exp(x), x <= 0: k = floor(x / ln 2 + 1/2), r = (x - k ln2_hi) - k ln2_lo, the Taylor polynomial of degree 13 by
 *       Horner, times 2^k through the exponent bits; 0 below -708.  Within 1 ulp of libm on [-50, 0].
 *   M7. outputs are floats rounded once from the doubles; rows in input order of the surviving points; src_index[row] = the
 *       input index (PCL's getCorrespondingIndices).  Normals are not flipped towards a viewpoint: the sign is eigen33's. */
typedef struct sfmhip_mls_opts {
  double search_radius;     /* r: finite and > 0 (the default 0 must be replaced) */
  int32_t polynomial_order; /* 0, 1 or 2 */
  int32_t compute_normals;  /* 0: out_normals4 is not written */
  double sqr_gauss_param;   /* g; <= 0: r r */
} sfmhip_mls_opts;
typedef struct sfmhip_mls_stats {
  int32_t n_out, n_dropped /* finite points with fewer than 3 neighbours */, n_plane_only, n_degenerate, n_fit_failed, max_neighbours;
} sfmhip_mls_stats;
/* radius 0 (must be set), order 2, normals on, gauss 0 */
int sfmhip_mls_default_opts(sfmhip_mls_opts* opts);
/* out_xyz: 3 n, out_normals4: n x (nx, ny, nz, curvature), src_index: n, stats: each may be NULL.  out_cloud: NULL, or it
 * receives a new handle on the same context over the smoothed points, which never leave the device.  SFMHIP_ERR_ARG with
 * nothing written for a NULL cloud, opts or n_out, a radius that is not finite and > 0, an order outside 0..2 or a non-finite
 * sqr_gauss_param.  No point, or no finite point: SFMHIP_OK, *n_out = 0. */
int sfmhip_cloud_mls(sfmhip_cloud* cloud, const sfmhip_mls_opts* opts, float* out_xyz, float* out_normals4, int32_t* src_index,
                     int32_t* n_out, sfmhip_mls_stats* stats, sfmhip_cloud** out_cloud);
/* With sfmhip_set_timing on (zeros while it is off): host-clock ms of the last call on this handle -- the radius grid (0 when
 * it was there already), the fit, the compaction with its downloads. */
int sfmhip_cloud_mls_last_timing(sfmhip_cloud* cloud, double ms3[3]);

/* ---- colour region growing and the dendrometry bounds (reference src/Segmentation.cpp:3-66, src/DendrometryE.cpp:3-29) ----
 * pcl::RegionGrowingRGB over the index list of a PassThrough, on the same device-resident cloud.  The rules (DESIGN.md
 * f-8 has them in full; parity UNPINNED, PCL is not in the image; + marks what is our reading):
 *   1. the options below; the three thresholds are stored squared, in float;
 *   2. every indexed point gets its min(region_neighbour_number, n_idx) nearest INDEXED points, itself included, in
 *      (d2, index) order +, d2 as above; a point outside the list (or non-finite +) has no list and is nobody's neighbour;
 *   3. colour difference: the integer sum of the squared differences of the 8-bit channels of 0x00RRGGBB;
 *   4. growth: seeds in list order; a flood (FIFO) from each unlabelled seed looks at the first neighbour_number
 *      entries of the current point u and takes an unlabelled v iff colour_diff(u, v) <= point threshold^2;
 *   5. segment neighbours: the minimum d2 over all entries of a segment's points to each other segment, the
 *      region_neighbour_number nearest kept, stored in descending (d2, segment) order; segment colour per channel
 *      unsigned(float(sum) / float(count));
 *   6. homogeneous merging in segment order over the stored lists (d2 > distance^2 skipped; an unlabelled neighbour
 *      joins iff its colour difference to THIS segment is < region threshold^2), then every region under
 *      min_cluster_size moves into the region of the nearest entry of its list (sorted by (d2, segment) +);
 *   7. clusters in region order after PCL's swap-with-last compaction of emptied regions +, then those outside
 *      [min_cluster_size, max_cluster_size] erased.
 * The index list must be strictly ascending (what sfmhip_cloud_passthrough writes); an empty or malformed list is
 * SFMHIP_ERR_ARG.  rgb: n packed colours as a PCD's rgb field holds them (the top byte is ignored). */
typedef struct {
  int32_t region_neighbour_number; /* 100 (1..128) */
  int32_t neighbour_number;        /* 30 */
  int32_t min_cluster_size;        /* 600 */
  int32_t max_cluster_size;        /* INT_MAX */
  float distance_threshold;        /* 10 */
  float point_color_threshold;     /* 6 */
  float region_color_threshold;    /* 5 */
} sfmhip_segment_opts;
typedef struct {
  int32_t n_idx;      /* indexed points that took part (the finite ones) */
  int32_t n_segments; /* segments the growth made */
  int32_t n_regions;  /* regions the homogeneous merging opened */
  int32_t rounds;     /* label-propagation rounds */
} sfmhip_segment_stats;
/* the reference's values (setDistanceThreshold(10), setPointColorThreshold(6), setRegionColorThreshold(5),
 * setMinClusterSize(600); PCL's defaults for the rest) */
void sfmhip_segment_default_opts(sfmhip_segment_opts* opts);
/* labels: n entries, the final cluster of every point of the cloud, -1 = in no cluster; cluster c lists its points in
 * ascending index.  *n_clusters = 0 is not an error here (the reference exits on it).  stats may be NULL. */
int sfmhip_cloud_segment_rgb(sfmhip_cloud* cloud, const uint32_t* rgb /* n */, const int32_t* indices, int n_idx,
                             const sfmhip_segment_opts* opts, int32_t* labels /* n */, int32_t* n_clusters,
                             sfmhip_segment_stats* stats);
/* staged: rule 2 alone.  idx / d2 are n_idx x k (k in 1..128), row r for indices[r]; idx holds cloud indices, -1 / +inf
 * where the list is shorter than k. */
int sfmhip_cloud_subset_knn(sfmhip_cloud* cloud, const int32_t* indices, int n_idx, int k, int32_t* idx, float* d2);
/* staged: rules 2-4.  segment: n entries, the growth's segment of every point (-1 outside the list). */
int sfmhip_cloud_segment_grow(sfmhip_cloud* cloud, const uint32_t* rgb, const int32_t* indices, int n_idx,
                              const sfmhip_segment_opts* opts, int32_t* segment /* n */, int32_t* n_segments,
                              int32_t* rounds);
/* host-clock ms of the last sfmhip_cloud_segment_rgb call on this handle: subset k-NN, growth, segment statistics,
 * the host's region step, the whole call. */
int sfmhip_cloud_segment_last_timing(sfmhip_cloud* cloud, double* ms5);
/* pcl::getMinMax3D over the finite points + (FLT_MAX / -FLT_MAX for none) and, if height is not NULL,
 * Dendrometry::estimate's "Total Height": the sqrt of the double sum of squares of the float differences. */
int sfmhip_cloud_minmax(sfmhip_cloud* cloud, float* mn /* 3 */, float* mx /* 3 */, double* height);

/* ---- dendrometry: the measurements Dendrometry::estimate leaves blank (reference src/DendrometryE.cpp:3-29) ----
 * Tree height along the vertical, diameter at breast height (DAP / DBH), the stem taper profile, crown base height, live
 * crown length and crown spread N-S / E-W of one tree's cloud.  The reference has no implementation; the contract is
 * this rule list, whose arithmetic is csrc/dendro.h (compiled by g++ and hipcc without contraction; the device equals the
 * host build bit for bit).
 *  1 options: the table below; lengths are metres and are divided by `scale` (metres per cloud unit) once, in f64.
 *    SFMHIP_ERR_ARG: |up| not 1 within 1e-6, north parallel to up, scale / slice / extent_bin not > 0, ransac_iters outside
 *    1..4096, r_min < 0, r_max < r_min, a negative tolerance, a non-finite dbh_height, extent_q outside (0, 1], crown_factor not > 0, min_inliers < 1,
 *    min_sectors outside 0..16, crown_run < 1, min_slice_pts < 3, an infinite ground.  north is projected off up and
 *    normalised; east = north x up.
 *  2 selection: the finite points (with labels: those with labels[i] == label, the layout sfmhip_cloud_segment_rgb writes)
 *    whose frame coordinates are finite floats.  Empty: status OK, flag bit 0, NaN outputs.
 *  3 frame: (e, n, h) = (east.p, north.p, up.p), each (a0 x + a1 y) + a2 z in f64, stored as float32.  h0 = ground / scale,
 *    or the least h of the selection when ground is NaN; total_height = (max h - h0) scale.  No point at or above h0: as
 *    empty.
 *  4 slices of thickness t: k = floor((h - h0) / t) in f64, h < h0 dropped; S = k of the top point + 1, at most 4096, the
 *    last slice takes what lies above it.  Within a slice the points keep ascending input index.
 *  5 circle RANSAC on (e, n) per slice of >= min_slice_pts points.  Iteration j draws three positions
 *    (u64(hash(seed, k, j, draw)) n_k) >> 32, hash = mix(mix(mix(mix(seed + 0x9E3779B9) ^ k) + 0x85EBCA6B ^ j) + 0xC2B2AE35 ^ draw)
 *    in u32 with mix(x): x ^= x >> 16, x *= 0x7FEB352D, x ^= x >> 15, x *= 0x846CA68B, x ^= x >> 16 (+ binds before ^);
 *    a repeated position skips the iteration.  Model: the circumcircle in f64 relative to the first point; skipped when the
 *    determinant is 0 or r is outside [r_min, r_max].  Inlier: |sqrt(dx^2 + dy^2) - r| <= tol in f64.  Arc cover: a 16-bit
 *    mask of the 22.5-degree sectors (counter-clockwise from +e) that hold inliers, from the signs of (dx, dy), |dx| against
 *    |dy| and the smaller against 0.41421356237309503 times the larger.  Winner: the largest key (count << 32) |
 *    (4095 - j) << 16 | mask over the iterations with an inlier.  Stem slice: count >= min_inliers and popcount(mask) >=
 *    min_sectors.
 *  6 refit of a stem slice on the winner's inliers (the set is not evaluated again): Kasa's algebraic fit in coordinates
 *    relative to the RANSAC centre, then exactly 10 Gauss-Newton steps on d_i - r (a singular or non-finite step changes
 *    nothing), then the RMS residual.  Each sum: point i of the slice adds to slot i mod 256 in ascending i, four 64-entry
 *    trees with strides 32..1, (w0 + w1) + (w2 + w3).
 *  7 DBH: x = dbh_height / t - 0.5, slices floor(x) and floor(x) + 1; both stem: radius and centre interpolated linearly
 *    with weight x - floor(x); one: that slice, flag bit 1; none: NaN, flag bit 2.  dbh = 2 r scale.
 *  8 extent of a slice: histogram of the distance to the vertical axis through the DBH centre, 1024 bins of extent_bin, the
 *    last takes the rest; the upper edge of the bin where the cumulative count reaches ceil(extent_q n_k) (at least 1).
 *  9 crown base: the lowest slice k with (k + 0.5) t > dbh_height whose crown_run slices k .. k + crown_run - 1 all exist,
 *    hold >= min_slice_pts points and have extent > crown_factor r_dbh.  crown_base_height = k t scale, live_crown =
 *    total_height - crown_base_height; none: NaN, flag bit 3.
 * 10 spread over the selected points with h >= h0 + k t (compared in f64): E-W = (max e - min e) scale, N-S likewise with n,
 *    max and min float32, the difference in f64.  NaN without a crown base. */
typedef struct sfmhip_dendro_opts {
  double up[3];          /* (0, 0, 1) */
  double north[3];       /* (0, 1, 0) */
  double scale;          /* 1: metres per cloud unit */
  double ground;         /* NaN: the lowest selected point; else the ground height along up, metres */
  double dbh_height;     /* 1.3 */
  double slice;          /* 0.1 */
  double inlier_tol;     /* 0.02 */
  double r_min, r_max;   /* 0.02, 1.5 */
  double extent_q;       /* 0.95 */
  double extent_bin;     /* 0.05 */
  double crown_factor;   /* 3 */
  int32_t ransac_iters;  /* 256; 1 ... 4096 */
  int32_t min_inliers;   /* 20 */
  int32_t min_sectors;   /* 6 of 16 */
  int32_t crown_run;     /* 3 */
  int32_t min_slice_pts; /* 10 */
  uint32_t seed;         /* 1 */
} sfmhip_dendro_opts;
typedef struct sfmhip_dendro_slice { /* one row of the stem taper table, cloud units; NaN where the slice is no stem slice */
  int32_t count;   /* points of the slice */
  int32_t stem;    /* 1: a stem slice */
  int32_t inliers; /* the winner's count (0: no hypothesis had an inlier) */
  int32_t mask;    /* ... and its sector mask */
  double ce, cn;   /* refitted centre (e, n) */
  double radius, rms;
  double extent;   /* rule 8 (NaN: empty slice, or no DBH axis) */
} sfmhip_dendro_slice;
typedef struct sfmhip_dendro_result { /* metres */
  double total_height, dbh, dbh_e, dbh_n /* the DBH centre */, crown_base_height, live_crown, spread_ns, spread_ew;
  double ground;             /* h0 scale */
  int32_t n_selected, n_slices;
  int32_t crown_base_slice;  /* -1: none */
  int32_t flags;             /* bit 0 empty selection, 1 DBH from one slice, 2 no DBH, 3 no crown base */
} sfmhip_dendro_result;
void sfmhip_dendro_default_opts(sfmhip_dendro_opts* opts);
/* labels: NULL (every finite point) or n entries. */
int sfmhip_cloud_dendrometry(sfmhip_cloud* cloud, const int32_t* labels, int32_t label, const sfmhip_dendro_opts* opts,
                             sfmhip_dendro_result* out);
/* The same call, returning the slice table: *n_slices rows exist, the first min(cap, *n_slices) are written; with out not
 * NULL, the scalars too (one run of the pipeline for both). */
int sfmhip_cloud_dendro_profile(sfmhip_cloud* cloud, const int32_t* labels, int32_t label, const sfmhip_dendro_opts* opts,
                                int cap, sfmhip_dendro_slice* slices, int32_t* n_slices, sfmhip_dendro_result* out);
/* host-clock ms of the last of these calls on the handle: frame + bounds, slice ordering, RANSAC, refit + table, extent + crown
 * + spread, the whole call.  Slice ordering and RANSAC are timed apart only under sfmhip_set_timing (a stream synchronisation
 * each); without it their device time shows in the refit's figure. */
int sfmhip_cloud_dendro_last_timing(sfmhip_cloud* cloud, double ms6[6]);

/* ---- the ground plane: the vertical frame the dendrometry needs ----
 * A structure-from-motion cloud stands in the first camera's frame: gravity points anywhere and the lowest point along z is
 * no ground.  This call finds the dominant ground plane of the cloud by RANSAC, refits it and orients it so that the trees
 * stand on it; sfmhip_dendro_opts_from_ground hands it to the dendrometry as up, north and ground.  Metric scale cannot
 * come from the cloud: it stays the caller's `scale` (a similarity registration against a metric cloud gives it:
 * sfmhip_cloud_register below).  The arithmetic is csrc/ground.h (compiled by g++ and hipcc without
 * contraction; the device equals the host build bit for bit).  The rules:
 *  1 selection: the finite points (with labels: those with labels[i] == label), listed in ascending input index (flag, the
 *    handle's scan, emit).  Fewer than 3: status OK, flag bit 0, every double NaN, winner -1.  SFMHIP_ERR_ARG: ransac_iters
 *    outside 1..4096, a negative or non-finite inlier_tol / inlier_rel, below_max outside [0, 1], a non-finite hint,
 *    max_tilt_deg outside (0, 180], refit_rounds outside 0..8, min_inliers < 3, n_cam < 0, n_cam > 0 without centres.
 *    An up_hint of length 0 is no hint; otherwise it is normalised once, hint / sqrt(hint . hint).
 *  2 tolerance: tol = inlier_tol if > 0, else inlier_rel sqrt((dx dx + dy dy) + dz dz) with d = (f64)max - (f64)min of the
 *    selection's float32 bounding box.
 *  3 hypothesis j draws three positions of the list, (u64(hash(seed, 0x67726E64, j, draw)) n_sel) >> 32 with f-11 rule 5's
 *    hash (csrc/draw_hash.h); a repeated position skips the iteration.  With the points a, b, c: u = b - a, v = c - a in f64,
 *    m = (u1 v2 - u2 v1, u2 v0 - u0 v2, u0 v1 - u1 v0), mm = (m0 m0 + m1 m1) + m2 m2; skipped when mm is 0 or not finite;
 *    n = m / sqrt(mm).  With a hint: skipped when |(n0 h0 + n1 h1) + n2 h2| < cos(max_tilt_deg pi / 180) (the host's cos, once).
 *  4 score, all integers: for every point of the list s = (n0 (x - a0) + n1 (y - a1)) + n2 (z - a2) in f64; inliers count
 *    |s| <= tol, pos counts s > tol, neg counts s < -tol.
 *  5 orientation: with camera centres, s as in rule 4: more centres with s > 0 than with s < 0 keeps n, fewer flips it, a tie
 *    falls through; then pos > neg keeps n, pos < neg flips it; still tied, the sign that makes the first non-zero
 *    component of n positive.  below = the count (pos or neg) on the side the oriented normal points away from.
 *  6 winner: admissible iff inliers >= min_inliers and below <= floor(below_max n_sel) (f64 product); the winner holds the
 *    largest 64-bit key inliers << 32 | (4095 - j).  None admissible: flag bit 1, NaN outputs (tol and n_selected stay),
 *    winner -1.
 *  7 refit, refit_rounds times: the inliers of the current plane; their centroid (three sums / N), then the six sums of
 *    products of (p - centroid) in f64, each / N: the 3 x 3 covariance.  The normal is the third row of Vt of csrc/jacobi.h's
 *    jacobi_svd<3, 3, 3, 3> on it, divided by its length, its sign flipped when its dot with the previous normal is < 0;
 *    the plane passes through the centroid.  Each sum: the point at list position i adds to slot i mod 256 in ascending i,
 *    non-inliers add nothing; four 64-entry trees with strides 32..1, then (w0 + w1) + (w2 + w3) (f-11 rule 6).  A round with
 *    fewer than 3 inliers or a non-finite normal or centroid keeps the previous plane and sets flag bit 2.  The
 *    orientation of rule 5 is decided once, on the winner, and every refit carries it.  inliers, above (s > tol), below
 *    (s < -tol) and rms = sqrt(sum of s s over the inliers / inliers) are those of the final plane, counted once more.
 *  8 frame: up = the final normal; offset = (up0 a0 + up1 a1) + up2 a2 with a the centroid (the winner's first point when
 *    refit_rounds is 0).  north = h - (h . up) up, normalised, with h = north_hint / |north_hint|; when that length is not
 *    > 1e-6 (or the hint is 0), h is the coordinate axis with the smallest |up| component (the lowest index on a tie) and
 *    flag bit 3 is set.
 * What the rules do not do: a scene whose largest plane is a wall at the edge of the cloud needs camera centres or an
 * up_hint; sloping ground gives the slope's normal, not gravity; one plane: the terrain over it is sfmhip_cloud_terrain's
 * (f-20, below). */
typedef struct sfmhip_ground_opts {
  double inlier_tol;      /* 0: use inlier_rel; else cloud units */
  double inlier_rel;      /* 0.005 of the selection's bounding-box diagonal */
  double below_max;       /* 0.01: share of the selection allowed further than tol on the far side of the plane */
  double up_hint[3];      /* (0,0,0): none */
  double max_tilt_deg;    /* 180: with a hint, hypotheses tilted further from it are skipped */
  double north_hint[3];   /* (0,1,0) */
  int32_t ransac_iters;   /* 512; 1 ... 4096 */
  int32_t min_inliers;    /* 100 */
  int32_t refit_rounds;   /* 2; 0 ... 8 */
  uint32_t seed;          /* 1 */
} sfmhip_ground_opts;
typedef struct sfmhip_ground_result {
  double up[3], north[3]; /* unit, north orthogonal to up */
  double offset;          /* up . p = offset on the plane, cloud units */
  double rms, tol;        /* of the final plane's inliers; the tolerance used */
  int32_t n_selected, inliers, below, above, winner /* iteration, -1 none */, flags;
} sfmhip_ground_result;
void sfmhip_ground_default_opts(sfmhip_ground_opts* opts);
/* labels: NULL (every finite point) or n entries; cam_centres: NULL or 3 n_cam doubles in the cloud's frame. */
int sfmhip_cloud_ground_plane(sfmhip_cloud* cloud, const int32_t* labels, int32_t label, const sfmhip_ground_opts* opts,
                              const double* cam_centres, int n_cam, sfmhip_ground_result* out);
/* host only: io->up, io->north and io->ground = offset * io->scale from a result that has a plane (SFMHIP_ERR_ARG otherwise) */
int sfmhip_dendro_opts_from_ground(const sfmhip_ground_result* ground, sfmhip_dendro_opts* io);
/* host-clock ms of the last sfmhip_cloud_ground_plane call on the handle: select + bounds + hypotheses, score, pick + refit,
 * the whole call.  The score is timed apart only under sfmhip_set_timing (a stream synchronisation each side); without it its
 * device time shows in the refit's figure. */
int sfmhip_cloud_ground_last_timing(sfmhip_cloud* cloud, double ms4[4]);

/* ---- individual trees: the stems of a plot and every point's tree ----
 * The dendrometry and the ground plane take `labels, label` to say which points are the tree.  This call makes such labels:
 * from the levelled cloud it finds the stems in a height band and gives every point above the ground the number of the
 * tree it belongs to, by shortest paths through the occupied voxels from the stems.  There is no reference
 * implementation; the contract is this rule list, whose arithmetic is csrc/trees.h (compiled by g++ and hipcc without
 * contraction).  Every result is an integer, or an f64 expression of integers written in one order, and none depends on
 * the order of evaluation: the device equals the host build byte for byte.
 *  1 options: the table below; lengths are metres and are divided by `scale` (metres per cloud unit) once, in f64.  The
 *    frame and its refusals are f-11 rule 1's (|up| not 1 within 1e-6, north parallel to up, scale not > 0).
 *    SFMHIP_ERR_ARG also: a non-finite ground; ground_clear < 0; band_lo < ground_clear; band_hi <= band_lo; stem_cell,
 *    voxel or max_stem_width not > 0 (in metres or in cloud units) or not finite; max_path < 0; min_cell_pts < 1;
 *    min_stem_pts < 1; max_trees outside 1..4096.
 *  2 selection and frame: f-11 rules 2 and 3.  Selected: the finite points (with labels_in: those with labels_in[i] ==
 *    label) whose frame coordinates (e, n, h) = (east.p, north.p, up.p), each (a0 x + a1 y) + a2 z in f64 stored as
 *    float32, are finite.  h0 = ground / scale.
 *  3 classes: with d = (f64)h - h0, a selected point is above (the set A) when d >= clear, and in the band (B, a subset
 *    of A) when lo <= d < hi.  Every point outside A gets tree -1.  A empty: status OK, flag bit 0, n_trees 0, all -1.
 *    e_min, n_min and the maxima of e, n, h are float32, over A.
 *  4 stem cells of size c: ix = floor(((f64)e - e_min) / c), iy likewise with n; De = ix of e_max + 1, Dn likewise;
 *    De Dn > 2^24 (as f64): SFMHIP_ERR_ARG.  A cell is occupied when it holds >= min_cell_pts points of B.  Cell id =
 *    iy De + ix.
 *  5 stems: the 8-connected components of the occupied cells; a component's id is its least cell id.  A component is a
 *    stem when it holds >= min_stem_pts points of B and (ix_max - ix_min + 1) c <= max_stem_width, likewise iy.  Stems are
 *    numbered 0..T-1 by ascending component id; beyond max_trees the first max_trees are kept and flag bit 2 is set.
 *    T = 0: flag bit 1, all -1, n_voxels 0.  Centre: with the i64 sums Se = sum count (2 ix + 1), Sn likewise and N = sum
 *    count over the component's cells, e = e_min + (c (f64)Se) / (f64)(2 N), n likewise;
 *    foot[a] = (e east[a] + n north[a]) + h0 up[a].
 *  6 voxels of size v over A: (vx, vy, vz) = floor of ((f64)e - e_min, (f64)n - n_min, (f64)h - h0) / v; the dimensions
 *    from the maxima; Dx Dy Dz >= 2^31 (as f64): SFMHIP_ERR_ARG (raise `voxel`).  Both caps are checked before any stem is
 *    looked for.  The graph's nodes are the occupied voxels, its edges the 26-neighbourhood, with integer weights 10 for a
 *    face step, 14 for an edge step, 17 for a corner step.
 *  7 seeds: a voxel that holds a point of B whose cell belongs to stem s is a seed of s at cost 0.
 *  8 labels: cost(v) = the least path weight from any seed; tree(v) = the lowest s among the stems whose seeds reach v at
 *    that cost; -1 for a voxel no seed reaches and, with max_path > 0, for one whose cost exceeds
 *    floor(10 (max_path / scale) / v).  This is the unique fixed point of key(v) = min(key(v), key(u) + w) over the edges
 *    with key = (cost, s) in lexicographic order.
 *  9 outputs: tree_of[i] = the tree of point i's voxel.  Stem row s: e, n, foot, cell_id (the component id), band_points
 *    (N), band_cells, points (the points with tree s).  n_labelled counts the points with a tree, max_cost is the largest
 *    cost of a voxel with a tree.
 * What the rules do not do: the method is a shortest-path partition of a voxel graph, not a crown model; crowns that
 * interpenetrate are split where the paths meet; a tree with no stem points in the band (an occluded one) is not found and
 * its points go to a neighbour or to -1; low vegetation that bridges two stems above ground_clear does not harm the
 * partition but ends up in somebody's tree. */
typedef struct sfmhip_trees_opts {
  double up[3];           /* (0, 0, 1) */
  double north[3];        /* (0, 1, 0) */
  double scale;           /* 1: metres per cloud unit */
  double ground;          /* required: the ground height along up, metres (sfmhip_trees_default_opts leaves NaN) */
  double ground_clear;    /* 0.3: points lower than this above the ground belong to no tree */
  double band_lo, band_hi; /* 1.0, 1.6: the band the stems are looked for in */
  double stem_cell;       /* 0.05 */
  double max_stem_width;  /* 1.5 */
  double voxel;           /* 0.15 */
  double max_path;        /* 0: unlimited */
  int32_t min_cell_pts;   /* 2 */
  int32_t min_stem_pts;   /* 30 */
  int32_t max_trees;      /* 4096; 1 ... 4096 */
  int32_t pad;
} sfmhip_trees_opts;
typedef struct sfmhip_tree_stem { /* cloud units */
  double e, n;      /* the stem's centre in the frame */
  double foot[3];   /* ... and on the ground plane, in the cloud's coordinates */
  int32_t cell_id, band_points, band_cells, points;
} sfmhip_tree_stem;
typedef struct sfmhip_trees_result {
  int32_t n_selected, n_above, n_band, n_trees, n_voxels, n_labelled, max_cost;
  int32_t flags; /* bit 0 nothing above the clearance, 1 no stem, 2 more stems than max_trees */
} sfmhip_trees_result;
void sfmhip_trees_default_opts(sfmhip_trees_opts* opts);
/* host only: io->up, io->north and io->ground = offset * io->scale from a result that has a plane (SFMHIP_ERR_ARG otherwise) */
int sfmhip_trees_opts_from_ground(const sfmhip_ground_result* ground, sfmhip_trees_opts* io);
/* labels_in: NULL (every finite point) or n entries; tree_of: n entries on the host, the layout sfmhip_cloud_dendrometry
 * takes as labels; out->n_trees stem rows exist, the first min(cap, n_trees) are written. */
int sfmhip_cloud_trees(sfmhip_cloud* cloud, const int32_t* labels_in, int32_t label, const sfmhip_trees_opts* opts, int32_t* tree_of,
                       int cap, sfmhip_tree_stem* stems, sfmhip_trees_result* out);
/* host-clock ms of the last sfmhip_cloud_trees call on the handle: frame + bounds, stems, voxels + neighbours, sweeps, labels,
 * the whole call; with sweeps not NULL, the sweeps it enqueued (a multiple of 16).  The voxel stage and the sweeps are timed
 * apart only under sfmhip_set_timing (a stream synchronisation); without it the voxel stage's device time shows in the sweeps'. */
int sfmhip_cloud_trees_last_timing(sfmhip_cloud* cloud, double ms6[6], int32_t* sweeps);

/* ---- the terrain model: ground points, a DTM raster, height above ground ----
 * The ground plane is one plane, and the trees and the dendrometry take one scalar `ground` along `up`.  On a plot that
 * undulates every height is then wrong by the plane's residual.  This call classifies the ground points with a progressive
 * morphological filter on a raster (Zhang et al. 2003; PCL 1.8.1's ApproximateProgressiveMorphologicalFilter), rasterises
 * a digital terrain model from them and replaces every point's height by its height above the terrain.  The tree and
 * dendrometry calls then run unchanged on the normalised cloud with up = +z, ground = 0.  PCL parity is UNPINNED; + marks a
 * reading of PCL from memory.  The arithmetic is csrc/terrain.h (compiled by g++ and hipcc without contraction): every step
 * is a min, a max or a comparison of float32 or f64 values, or an f64 expression written in one order, so the device equals
 * the host build byte for byte.  The rules:
 *  1 options: the table below; lengths are metres and are divided by `scale` once, in f64.  The frame and its refusals are
 *    f-11 rule 1's.  SFMHIP_ERR_ARG also: cell, initial_distance or max_distance not > 0 or not finite (in metres or in
 *    cloud units); max_window or slope negative or not finite; base < 2; fill_rounds outside 0..4096; relax_sweeps outside
 *    0..1024.
 *  2 selection and frame: f-13 rule 2's (e, n, h) as float32; selected: finite in both forms, labels == label when labels
 *    are given.  Nothing selected: status OK, flag bit 0, De = Dn = 0, every per-point output "not ground / NaN".
 *  3 raster: c = cell / scale; e_min, n_min and the maxima are float32, over the selection; ix = floor(((f64)e - e_min) / c),
 *    iy likewise with n; De = ix(e_max) + 1, Dn likewise; De Dn > 2^24 (as f64): SFMHIP_ERR_ARG.  Cell id = iy De + ix.
 *  4 lowest-point raster: Z_0[cell] = the least h of the cell's selected points; a cell without points is empty.
 *  5 windows +: k_i = base^i when exponential, else (i + 1) base, for i = 0, 1, ... (an integer, held as an f64: exact below
 *    2^53); window i exists while (f64)(2 k_i + 1) <= (max_window / scale) / c and i < 32.  dh_0 = d0;
 *    dh_i = min(dmax, slope ((f64)(2 (k_i - k_{i-1})) c) + d0), with d0 and dmax the two distances over scale.  No window:
 *    flag bit 2, and every selected point is a ground point.
 *  6 opening of Z_i by window i: E_i[x, y] = the least non-empty Z_i[x', y'] with |x' - x| <= k_i, |y' - y| <= k_i inside
 *    the raster, empty when there is none; O_i = the largest non-empty E_i over the same window, empty when there is none;
 *    Z_{i+1} = O_i.
 *  7 ground points: a selected point in cell q is a ground point iff (f64)h - (f64)O_i[q] <= dh_i for every window i.
 *  8 terrain raster: for a cell with m > 0 ground points T = float32(S / (f64)m); S is their (f64)h summed in this order:
 *    the point at position j of the cell's run (its selected points in ascending input index) adds to slot j mod 64 in
 *    ascending j, points that are not ground add nothing; the 64 slots then fold by strides 32, 16, ..., 1
 *    (slot[s] += slot[s + stride]).  The cell gets kind 1.
 *  9 fill: in round r = 1 .. fill_rounds every cell that is empty before the round and has a non-empty 8-neighbour takes
 *    float32(s / (f64)m), s the f64 sum (from 0) of those neighbours' values before the round in the order (dx, dy) =
 *    (-1,-1), (0,-1), (1,-1), (-1,0), (1,0), (-1,1), (0,1), (1,1), m their count; it gets kind 2.  The fill stops after a
 *    round that fills nothing (that round is counted).  Cells still empty: kind 0, value NaN, flag bit 1.
 * 10 relaxation: relax_sweeps Jacobi sweeps over the kind-2 cells, kind-1 cells fixed: each becomes
 *    float32(((W + E) + (S + N)) / 4.0) in f64 from the previous sweep's values (W, E: x - 1, x + 1; S, N: y - 1, y + 1);
 *    a neighbour outside the raster or of kind 0 counts as the cell's own value.
 * 11 height above ground of a selected point in cell q: NaN when q has kind 0.  Else u = ((f64)e - e_min) / c - 0.5,
 *    x0 = clamp(floor(u), 0, De - 1), x1 = min(x0 + 1, De - 1), fx = clamp(u - x0, 0, 1); v, y0, y1, fy likewise with n.
 *    The four corners T[y][x] are read as f64, a corner of kind 0 replaced by T[q];
 *    g = ((T00 (1 - fx) + T01 fx) (1 - fy)) + ((T10 (1 - fx) + T11 fx) fy); hag = float32((f64)h - g).
 * 12 canopy raster: chm[cell] = the largest finite hag of the cell's selected points, NaN when there is none.
 * 13 outputs: per point is_ground (0 / 1; 0 when not selected) and hag (NaN when not selected); the rasters T, kind and
 *    chm, row-major with ix fastest; the result below.  The normalised cloud has n rows: (e, n, hag) for a selected point
 *    with finite hag, three NaN otherwise, so a tree_of computed on it indexes the original cloud.
 * What the rules do not do: the opening's windows are clipped at the raster's edge, so a band of k_i cells along an
 * upslope edge is flattened (the opening of a plane is the plane only k cells inside); initial_distance must cover the
 * terrain's height change across one cell plus the noise; trunk points within initial_distance of the terrain are ground
 * points; with the ground plane's normal as `up` the model describes the undulation over the slope, not gravity. */
typedef struct sfmhip_terrain_opts {
  double up[3];            /* (0, 0, 1) */
  double north[3];         /* (0, 1, 0) */
  double scale;            /* 1: metres per cloud unit */
  double cell;             /* 0.5 */
  double max_window;       /* 9.0: the widest window, 2 k + 1 cells */
  double slope;            /* 1.0 */
  double initial_distance; /* 0.15 */
  double max_distance;     /* 2.5 */
  int32_t base;            /* 2 */
  int32_t exponential;     /* 1 */
  int32_t fill_rounds;     /* 64; 0 ... 4096 */
  int32_t relax_sweeps;    /* 32; 0 ... 1024 */
} sfmhip_terrain_opts;
typedef struct sfmhip_terrain_result {
  double c;                /* the cell, cloud units */
  float e_min, n_min;      /* the raster's origin in the frame */
  float t_min, t_max;      /* the least and largest T (NaN: no cell has a value) */
  float hag_max;           /* the largest finite hag (NaN: none) */
  int32_t De, Dn, n_selected, n_ground, n_windows;
  int32_t n_kind1, n_kind2, n_kind0; /* cells with ground points, filled, still empty */
  int32_t fill_rounds;     /* the fill rounds run */
  int32_t flags;           /* bit 0 nothing selected, 1 cells left empty, 2 no window */
  int32_t pad;
} sfmhip_terrain_result;
void sfmhip_terrain_default_opts(sfmhip_terrain_opts* opts);
/* host only: io->up and io->north from a result that has a plane (SFMHIP_ERR_ARG otherwise) */
int sfmhip_terrain_opts_from_ground(const sfmhip_ground_result* ground, sfmhip_terrain_opts* io);
/* labels: NULL (every finite point) or n entries; is_ground, hag: NULL or n entries on the host. */
int sfmhip_cloud_terrain(sfmhip_cloud* cloud, const int32_t* labels, int32_t label, const sfmhip_terrain_opts* opts,
                         int32_t* is_ground, float* hag, sfmhip_terrain_result* out);
/* the rasters of the last sfmhip_cloud_terrain call on the handle (De Dn entries each, any pointer may be NULL);
 * SFMHIP_ERR_ARG when there was no call. */
int sfmhip_cloud_terrain_raster(sfmhip_cloud* cloud, float* dtm, uint8_t* kind, float* chm);
/* the normalised cloud of the last call as a handle born on the device (as sfmhip_cloud_select's): the points never pass
 * through the host.  SFMHIP_ERR_ARG when there was no call. */
int sfmhip_cloud_terrain_normalize(sfmhip_cloud* cloud, sfmhip_cloud** out);
/* host-clock ms of the last sfmhip_cloud_terrain call on the handle: frame + raster, windows, point test + terrain raster,
 * fill + relax, heights + canopy, the whole call.  The windows and the point test are timed apart only under
 * sfmhip_set_timing (a stream synchronisation each); without it their device time shows in the fill's figure. */
int sfmhip_cloud_terrain_last_timing(sfmhip_cloud* cloud, double ms6[6]);

/* ---- crown delineation: tree tops and crowns from the canopy raster ----
 * sfmhip_cloud_trees finds a tree by its stem; a cloud taken from above has dense crowns and few stem points.  This call
 * finds the trees on the canopy height model instead: tree tops as variable-window maxima of the smoothed raster, crowns by
 * steepest ascent to a summit and window merging of the summits, then a tree number per point in the layout
 * sfmhip_cloud_dendrometry takes as labels.  The arithmetic is csrc/crowns.h (compiled by g++ and hipcc without
 * contraction).  Every quantity is a pure function of the raster and no result depends on the order in which cells are
 * visited, so the device equals the host build byte for byte.  PCL and the reference have nothing comparable: there is no
 * parity to pin.  The rules:
 *  1 options: the table below; lengths are metres and are divided by `scale` once, in f64.  SFMHIP_ERR_ARG: any of them not
 *    finite; scale, min_height, r_min or max_crown_radius not > 0; r_max < r_min; win_b < 0; crown_frac outside [0, 1];
 *    ground_clear < 0; smooth_passes outside 0..64; max_trees outside 1..65536; the cell c not > 0 or not finite;
 *    (r_max / scale) / c > 64, the window's cap in cells.
 *  2 input: a raster Z[Dn][De] of float32, row-major with ix fastest, cell id q = iy De + ix, the cell c in cloud units; NaN
 *    means empty.  De Dn > 2^24: SFMHIP_ERR_ARG.  De Dn = 0: status OK, flag bit 0.
 *  3 smoothing: H_0 = Z; pass p gives a non-empty cell H_{p+1} = float32(S / W), S the f64 sum (from 0) of k (f64)H_p and W
 *    the f64 sum of k over the non-empty cells of the 3 x 3 block inside the raster in the order (dx, dy) = (-1,-1), (0,-1),
 *    (1,-1), (-1,0), (0,0), (1,0), (-1,1), (0,1), (1,1) with k = 1, 2, 1, 2, 4, 2, 1, 2, 1.  An empty cell stays empty.
 *    H is the raster after smooth_passes passes.
 *  4 canopy: a cell is canopy iff H is finite and (f64)H >= min_height / scale.
 *  5 order: key(q) = (H[q], -q): the greater H wins, at equal H the smaller cell id.  Strict and total.
 *  6 ascent: up(q) = the canopy cell of greatest key among q and its 8 neighbours inside the raster; a canopy cell with
 *    up(q) = q is a summit; root(q) = the summit reached by following up (the key rises strictly).
 *  7 windows: for a summit s, r = min(r_max, max(r_min, win_a + win_b ((f64)H[s] scale))), rc = (r / scale) / c,
 *    R2 = max(2, (int)floor(rc rc)); dom(s) = the canopy cell of greatest key among the cells inside the raster with
 *    dx^2 + dy^2 <= R2, s included; parent(s) = root(dom(s)).  s is a top iff dom(s) = s; otherwise parent(s)'s key exceeds
 *    s's, so following parent ends at a top, top(s).
 *  8 numbering: tops are numbered 0 .. T - 1 by ascending cell id; beyond max_trees the first max_trees are kept and flag
 *    bit 2 is set; cells whose top was dropped get -1.
 *  9 crowns: a canopy cell q with t = top(root(q)) kept as number j has label j iff (f64)H[q] >= crown_frac (f64)H[t] and
 *    (f64)(dx^2 + dy^2) <= floor(mr mr), mr = (max_crown_radius / scale) / c, (dx, dy) from t to q.  Else -1; a cell that is
 *    not canopy has -1.
 * 10 points (cloud entry): tree_of[i] = label(cell of i) when point i was selected by the terrain call, its hag is finite
 *    and (f64)hag >= ground_clear / scale; else -1.  The cell of i is f-20 rule 3's.
 * 11 outputs: the top rows and the result below.  A top's e = e_min + ((f64)ix + 0.5) c, n likewise; height = Z[cell], the
 *    raw canopy in cloud units; height_smooth = H[cell]; cells = the cells with its label; points = the points with its
 *    number (0 from the raster entry); area = (f64)cells (c c).  max_depth = the most parent steps from a summit to its top.
 * What the rules do not do: this is a steepest-ascent partition with window merging, not a flooding watershed.  Two crowns
 * that touch are split along the valley of the smoothed raster.  A minor summit goes to the tree of the highest cell in its
 * window, which can leave a crown in two pieces.  A tree shorter than a taller neighbour's window away from it is absorbed. */
typedef struct sfmhip_crowns_opts {
  double scale;            /* 1: metres per cloud unit */
  double min_height;       /* 2.0: a cell lower than this is not canopy */
  double win_a;            /* 0.6: the window radius r = clamp(win_a + win_b * height in metres, r_min, r_max) */
  double win_b;            /* 0.06 */
  double r_min;            /* 0.6 */
  double r_max;            /* 5.0 */
  double crown_frac;       /* 0.3: a crown cell is at least this share of its top */
  double max_crown_radius; /* 10.0 */
  double ground_clear;     /* 0.3: points lower than this belong to no tree */
  int32_t smooth_passes;   /* 2; 0 ... 64 */
  int32_t max_trees;       /* 4096; 1 ... 65536 */
} sfmhip_crowns_opts;
typedef struct sfmhip_crown_top { /* cloud units */
  double e, n;             /* the centre of the top's cell in the frame */
  double area;             /* cells * c * c */
  float height;            /* Z[cell]: the raw canopy */
  float height_smooth;     /* H[cell] */
  int32_t cell_id, ix, iy, R2, cells, points;
} sfmhip_crown_top;
typedef struct sfmhip_crowns_result {
  double c;                /* the cell, cloud units */
  float e_min, n_min;      /* the raster's origin in the frame */
  int32_t De, Dn, n_canopy, n_summits;
  int32_t n_trees;         /* the tops, before the cap */
  int32_t n_labelled_cells, n_labelled; /* cells and points with a tree */
  int32_t max_depth;       /* the longest parent chain */
  int32_t flags;           /* bit 0 no canopy cell, 2 more tops than max_trees */
  int32_t pad;
} sfmhip_crowns_result;
void sfmhip_crowns_default_opts(sfmhip_crowns_opts* opts);
/* the raster entry: a host raster chm (De Dn floats, NULL when De Dn = 0) of any canopy model, e_min = n_min = 0.  labels,
 * smooth: NULL or De Dn entries on the host; min(n_trees, max_trees) top rows exist, the first min(cap, that) are written. */
int sfmhip_chm_crowns(sfmhip_ctx* ctx, const float* chm, int De, int Dn, double c, const sfmhip_crowns_opts* opts, int32_t* labels,
                      float* smooth, int cap, sfmhip_crown_top* tops, sfmhip_crowns_result* out);
/* the product: on the canopy raster, the frame coordinates and the heights above ground of the last sfmhip_cloud_terrain call
 * on the handle, where they lie on the device (SFMHIP_ERR_ARG when there was no such call); c, e_min and n_min are that
 * call's.  tree_of: NULL or n entries on the host.  Nothing but tree_of, the top rows and the result crosses to the host. */
int sfmhip_cloud_crowns(sfmhip_cloud* cloud, const sfmhip_crowns_opts* opts, int32_t* tree_of, int cap, sfmhip_crown_top* tops,
                        sfmhip_crowns_result* out);
/* the rasters H and label of the last sfmhip_cloud_crowns call on the handle (De Dn entries each, either pointer may be
 * NULL); SFMHIP_ERR_ARG when there was no call. */
int sfmhip_cloud_crowns_raster(sfmhip_cloud* cloud, float* smooth, int32_t* labels);
/* host-clock ms of the last sfmhip_cloud_crowns call on the handle: smoothing, ascent (up, doubling, the summit list),
 * windows (with the summit forest and the numbering), labels, points, the whole call.  The stages are timed apart only
 * under sfmhip_set_timing (a stream synchronisation each); without it the smoothing's device time shows in the ascent's. */
int sfmhip_cloud_crowns_last_timing(sfmhip_cloud* cloud, double ms6[6]);
/* the doubling rounds the last sfmhip_cloud_crowns call counted until one moved nothing: of rule 6's ascent, of rule 7's parents */
int sfmhip_cloud_crowns_last_rounds(sfmhip_cloud* cloud, int32_t rounds2[2]);

/* ---- two clouds meet: nearest points, rigid and similarity ICP ----
 * What pcl::IterativeClosestPoint with TransformationEstimationSVD / ...SVDScale computes, and pcl::transformPointCloud, on
 * two device-resident clouds of one context.  A similarity registration against a metric cloud is where the `scale` of the
 * dendrometry comes from.  The arithmetic is csrc/register.h (compiled by g++ and hipcc without contraction; the device equals
 * the host build bit for bit).  PCL parity is UNPINNED (PCL is not in the image); + marks a reading of PCL from memory.
 *  1 refusals: SFMHIP_ERR_ARG for handles of different contexts, a transform with a non-finite entry or scale not > 0,
 *    max_dist NaN or <= 0, eps < 0 or NaN, max_iters < 0, min_pairs < 3.  source == target is allowed.  An empty source or a
 *    target without a finite point: status OK, no pairs, mse NaN, flag FEW.
 *  2 moving a point, in f64: y_r = scale * ((R[3r] x + R[3r+1] y) + R[3r+2] z) + t_r, q = (float)y.  A source point that is
 *    non-finite before or after has no pair: idx -1, d2 +inf.  Every iteration moves the ORIGINAL floats by the current
 *    transform: the source is never changed and no product of increments accumulates.
 *  3 a pair: the finite target point of least (d2, index), d2 the family's float ((dx dx) + dy dy) + dz dz of q - target;
 *    duplicates resolve to the lower index.  Kept iff d2 <= (float)(max_dist * max_dist), squared in f64 +; +inf keeps all.
 *  4 sums, all f64, over source indices in consecutive blocks of 256: each block by the fixed-order tree of f-9 (a point
 *    without a pair adds +0.0), the block partials added sequentially in ascending order.  Pass 1: N, sum p, sum m (p the
 *    source float, m the matched target float, widened); mu_p = sum p / N, mu_m = sum m / N.  Pass 2: H[r][c] = sum (m_r -
 *    mu_m_r)(p_c - mu_p_c), sigma = sum ((dx dx + dy dy) + dz dz) of p - mu_p, and sum (double)d2.
 *  5 the estimate (Umeyama / Horn +): svd3(H) -> U, W, Vt (the 3 x 3 Jacobi of the pose step); d = +1 when det(U) det(Vt)
 *    >= 0, else -1; R[r][c] = (U[r][0] Vt[0][c] + U[r][1] Vt[1][c]) + (d U[r][2]) Vt[2][c]; scale = with_scale ? ((W0 + W1) +
 *    d W2) / sigma : the initial scale; t_r = mu_m_r - scale ((R[r][0] mu_p_0 + R[r][1] mu_p_1) + R[r][2] mu_p_2).
 *    DEGENERATE when svd3 raises its flag, sigma == 0, W1 <= 1e-12 W0 (pairs on a line), or the new scale or any entry of
 *    the new transform is not finite or the scale not > 0: the loop stops and the current transform is returned.
 *  6 the loop: T_0 = init.  For k = 0, 1, ...: C_k = the pairs under T_k (the idx array, -1 included).  pairs < min_pairs:
 *    flag FEW, stop (so FEW says of every returned transform that it has too few pairs, also with max_iters 0).  Else if
 *    k > 0 and C_k == C_{k-1}: converged 1, stop (the estimate would reproduce T_k).  Else if k > 0, eps > 0 and no entry
 *    of scale R and of t differs between T_k and T_{k-1} by more than eps: converged 2, stop.  Else if k == max_iters:
 *    converged 0, stop.  Else T_{k+1} = rule 5 on C_k, or stop with DEGENERATE.  iterations = k; pairs, mse (the mean of
 *    (double)d2 over the pairs; NaN without) and idx always describe the returned transform.
 *  7 sfmhip_cloud_nearest is rules 2 + 3 once, per source point.  A rejected pair reports idx -1 and keeps the d2 of its
 *    nearest point, so a cloud-to-cloud distance map is max_dist = +inf and sqrt(d2).  (Inside sfmhip_cloud_register the
 *    search of a point with nothing within max_dist ends there; its d2 is not reported.)
 *  8 sfmhip_cloud_transform writes q of rule 2 for every point (a non-finite point stays as it is) into a new handle born on
 *    the device; sfmhip_cloud_concat copies a's points, then b's, device to device.  Both keep the input order. */
typedef struct sfmhip_transform {
  double R[9];
  double t[3];
  double scale;
} sfmhip_transform; /* x -> scale R x + t, R row-major */
typedef struct sfmhip_register_opts {
  int32_t max_iters;  /* 50; 0: evaluate the initial transform only */
  int32_t with_scale; /* 0: rigid, the scale stays the initial one; 1: similarity */
  int32_t min_pairs;  /* 3 */
  int32_t reserved;
  double max_dist; /* +inf: every pair kept; else target cloud units, > 0 */
  double eps;      /* 0: off; else stop when no entry of scale R and t moved by more than eps */
} sfmhip_register_opts;
typedef struct sfmhip_register_result {
  sfmhip_transform T;
  int32_t iterations, pairs;
  int32_t converged; /* 0 limit (or a flag), 1 fixed point, 2 eps */
  int32_t flags;     /* 1 FEW, 2 DEGENERATE */
  double mse;        /* mean of (double)d2 over the pairs under T; NaN without pairs */
} sfmhip_register_result;
void sfmhip_register_default_opts(sfmhip_register_opts* opts);
/* T: NULL for the identity; idx / d2: one entry per source point */
int sfmhip_cloud_nearest(sfmhip_cloud* target, sfmhip_cloud* source, const sfmhip_transform* T, double max_dist, int32_t* idx,
                         float* d2);
/* opts: NULL for the defaults; init: NULL for the identity; idx: NULL or one entry per source point, the pairs under out->T */
int sfmhip_cloud_register(sfmhip_cloud* target, sfmhip_cloud* source, const sfmhip_register_opts* opts, const sfmhip_transform* init,
                          sfmhip_register_result* out, int32_t* idx);
int sfmhip_cloud_transform(sfmhip_cloud* cloud, const sfmhip_transform* T, sfmhip_cloud** out);
int sfmhip_cloud_concat(sfmhip_cloud* a, sfmhip_cloud* b, sfmhip_cloud** out);
/* With sfmhip_set_timing on (zeros while it is off): host-clock ms of the last sfmhip_cloud_register call with this target,
 * summed over its iterations -- search, sums, update + the record's read -- and the iterations it ran. */
int sfmhip_cloud_register_last_timing(sfmhip_cloud* target, double ms3[3], int32_t* iterations);

/* ---- coarse plot alignment: height-keyed pose voting and multi-start ICP ----
 * sfmhip_cloud_register needs `init` within a few degrees.  Two reconstructions of one plot differ by an arbitrary rotation,
 * translation and scale; once each is levelled by its ground plane, what is left is a scale, a yaw about the vertical and a
 * horizontal shift.  The points above the ground vote for those by their heights, ICP runs from every candidate at once, and
 * the start that pairs most wins.  The arithmetic is csrc/align.h (compiled by g++ and hipcc without contraction; integer
 * counts, f64 expressions in one written order: the device equals the host build byte for byte).
 * Entry 1, sfmhip_cloud_register_batch: n_init starts in one lock-step loop.  results[b] and row b of idx are byte-equal to
 *    what sfmhip_cloud_register(target, source, opts, &inits[b], ...) returns.  SFMHIP_ERR_ARG, nothing written: whatever
 *    f-17 rule 1 refuses for any one init, inits NULL, n_init outside 1..1024.  The launches per iteration do not depend on
 *    n_init; a large source is not walked in cell order (results do not depend on it).
 * Entry 2, sfmhip_cloud_align_vote, the rules:
 *  V1 SFMHIP_ERR_ARG: a frame f-11 rule 1 refuses (|up| not 1 within 1e-6, north parallel to up) or with a non-finite offset,
 *     an option outside its range below or non-finite, handles of different contexts, one handle given twice.
 *  V2 (e, n, h) per cloud by f-11 rules 2 and 3, float32; d = (f64)h - offset; hmax the largest d over the finite points; a
 *     point is above the ground iff d >= clear_rel hmax.  A side without an above point or with hmax <= 0: status OK, flag
 *     bit 0, no candidates.
 *  V3 the above points in ascending input index, every stride-th kept: stride = ceil(N_above / K).
 *  V4 tables, by the host: s_k = scale_lo (scale_hi / scale_lo)^(k / (n_scale - 1)), s_0 = scale_lo; cos and sin of 2 pi m / n_yaw.
 *  V5 hypothesis (k, m) moves source sample i to qe = s (c e - sn n), qn = s (sn e + c n), hq = s d.
 *  V6 W = window_rel max(e extent, n extent) of the target sample; centre = the midpoint 0.5 (min + max) of the target
 *     sample's (e, n) box minus that of q's box; lo = centre - W; w = 2 W / bins.
 *  V7 pair (i, j) votes iff |d_j - hq_i| <= h_tol, in bin floor(((e_j - qe_i) - lo_e) / w) and likewise for n, iff both lie
 *     in [0, bins).
 *  V8 a hypothesis's peak: its largest count, the lowest bin id by bins + bx on a tie; without a vote it is dropped.  The
 *     translation is lo + (b + 0.5) w per axis.
 *  V9 candidates by (votes descending, k ascending, m ascending), the first n_cand.  In cloud coordinates R = E_t^T (Rz E_s),
 *     t = E_t^T (te, tn, offset_t - s offset_s), scale = s, E's rows east, north, up; every entry (a0 b0 + a1 b1) + a2 b2.
 * Entry 3, sfmhip_cloud_align: V1 - V9; the source sample gathered by sfmhip_cloud_select (ground points are left out: a
 *    plane sliding on a plane pairs everything); entry 1 from the candidates against the whole target with with_scale =
 *    (n_scale > 1), max_iters = icp_max_iters, max_dist = icp_dist_bins w; the winner is the result with flags == 0 first by
 *    (pairs descending, mse ascending, candidate index ascending).  None: flag bit 1, the identity.  The caller hands the
 *    winner's T to sfmhip_cloud_register on the full clouds as init.
 * Limits: both clouds must be levelled (one dominant ground plane each); near-symmetric plots can tie; the scale range is
 * the caller's (the ratio of the two hmax is a guess when both clouds show the same tallest tree). */
typedef struct sfmhip_frame {
  double up[3], north[3]; /* as sfmhip_ground_result's */
  double offset;          /* up . p = offset on the ground, cloud units */
} sfmhip_frame;
typedef struct sfmhip_align_opts {
  double scale_lo, scale_hi; /* required: 0 < scale_lo <= scale_hi */
  double clear_rel;          /* 0.1; 0 <= value < 1 */
  double h_tol;              /* required: target units, > 0 */
  double window_rel;         /* 1; > 0 */
  double icp_dist_bins;      /* 1.25; > 0: entry 3's max_dist in vote bins */
  int32_t n_scale;           /* 15; 1 ... 64, 1 means scale_lo only */
  int32_t n_yaw;             /* 72; 1 ... 720 */
  int32_t bins;              /* 64; 4 ... 128 */
  int32_t src_samples;       /* 2048; 1 ... 8192 */
  int32_t tgt_samples;       /* 2048; 1 ... 8192 */
  int32_t n_cand;            /* 64; 1 ... 1024 */
  int32_t icp_max_iters;     /* 30; >= 0 */
  int32_t reserved;
} sfmhip_align_opts;
typedef struct sfmhip_align_candidate {
  sfmhip_transform T; /* source cloud -> target cloud */
  int32_t votes, k, m, bin;
} sfmhip_align_candidate;
typedef struct sfmhip_align_stats {
  double hmax_src, hmax_tgt; /* NaN for a cloud without a finite point */
  double w, window;          /* the bin width and W; NaN when flag bit 0 is set */
  int32_t n_above_src, n_above_tgt, n_src, n_tgt /* sample sizes */, n_hyp /* hypotheses with votes */;
  int32_t flags; /* 1 EMPTY */
} sfmhip_align_stats;
typedef struct sfmhip_align_result {
  sfmhip_register_result reg;  /* the winner's */
  sfmhip_align_candidate cand; /* the candidate it started from */
  int32_t cand_index;          /* its row, -1 none */
  int32_t n_same;              /* candidates whose ICP reached the winner's transform, byte for byte */
  int32_t n_cand;
  int32_t flags; /* 1 EMPTY, 2 NO_WINNER */
  sfmhip_align_stats stats;
} sfmhip_align_result;
void sfmhip_align_default_opts(sfmhip_align_opts* opts);
/* host only: up, north and offset of a ground result that has a plane (SFMHIP_ERR_ARG otherwise) */
int sfmhip_frame_from_ground(const sfmhip_ground_result* ground, sfmhip_frame* out);
/* opts: NULL for the defaults; results: n_init entries; idx: NULL or n_init rows of one entry per source point */
int sfmhip_cloud_register_batch(sfmhip_cloud* target, sfmhip_cloud* source, const sfmhip_register_opts* opts, const sfmhip_transform* inits,
                                int n_init, sfmhip_register_result* results, int32_t* idx);
/* as sfmhip_cloud_register_last_timing, of the last batch with this target; iterations: those of its longest problem */
int sfmhip_cloud_register_batch_last_timing(sfmhip_cloud* target, double ms3[3], int32_t* iterations);
/* candidates: room for opts->n_cand; n_out: how many were written */
int sfmhip_cloud_align_vote(sfmhip_cloud* target, sfmhip_cloud* source, const sfmhip_frame* target_frame, const sfmhip_frame* source_frame,
                            const sfmhip_align_opts* opts, sfmhip_align_candidate* candidates, int32_t* n_out, sfmhip_align_stats* stats);
int sfmhip_cloud_align(sfmhip_cloud* target, sfmhip_cloud* source, const sfmhip_frame* target_frame, const sfmhip_frame* source_frame,
                       const sfmhip_align_opts* opts, sfmhip_align_result* out);
/* host-clock ms of the last vote or alignment with this target: the vote, the batch ICP (0 after a vote alone), the whole call */
int sfmhip_cloud_align_last_timing(sfmhip_cloud* target, double ms3[3]);

/* ---- point-to-plane, trimmed and one-to-one ICP ----
 * A second registration entry beside sfmhip_cloud_register: the same search, the same loop record and the same batch, with
 * rejectors between the search and the sums and a second estimator.  The arithmetic is csrc/register_icp.h (compiled by g++
 * and hipcc without contraction; the device equals the host build bit for bit).  PCL parity is UNPINNED.
 *  1 refusals: whatever f-17 rule 1 refuses; trim outside (0, 1] or NaN; metric or one_to_one not 0 or 1; normal_stride not 3
 *    or 4; metric 1 without normals or with eps not > 0; min_pairs below the unknowns (3 for metric 0; 6, with scale 7, for
 *    metric 1).  Empty inputs as in f-17 rule 1.
 *  2 the search: f-17 rules 2 - 3 (the nearest finite target point by (d2, index), the source's cell order, max_dist).
 *  3 no plane (metric 1): a pair whose target normal has a non-finite component or is exactly (0, 0, 0) is dropped.  Normals
 *    are used as given (not renormalised) and uploaded once per call.
 *  4 one-to-one: among the surviving sources that chose target j only the one of least (d2, source index) survives.
 *  5 trim: N survivors; K = ceil(trim N) in f64, at least 1 when N >= 1; tau = the K-th smallest d2; every survivor with
 *    d2 <= tau is kept (ties at tau all stay: the kept count can exceed K).  N = 0 or trim = 1: tau = +inf.
 *  6 a dropped pair reports idx -1; pairs, mse, plane_mse and trim_d2 describe the kept set under the returned transform.
 *  7 metric 0: f-17 rules 4 - 6 on the kept pairs (the fixed-point stop: the kept set did not change).  With trim = 1 and
 *    one_to_one = 0 the call returns sfmhip_cloud_register's bytes.
 *  8 metric 1, the step: c = 0.5 (lo + hi) of the target's finite box, f64.  Per kept pair q (the moved source float), m, n
 *    widened: r = (n0 (q0 - m0) + n1 (q1 - m1)) + n2 (q2 - m2); qt = q - c; the row a = (qt x n, n, with_scale ? (n0 qt0 + n1
 *    qt1) + n2 qt2 : 0).  One pass of f64 sums in f-17 rule 4's order: N, a_i a_j (i <= j), a_i r, r r, (double)d2.  (a^T a) x
 *    = -(a^T r) by Cholesky in one written order (csrc/register_icp.h, plane_solve); DEGENERATE when a pivot is not > 1e-12
 *    times the largest diagonal entry or anything is non-finite (a target that is one plane is).  omega = x[0..2]: v = omega /
 *    2, vv = (v0 v0 + v1 v1) + v2 v2, dR = I + (2 (1 / (1 + vv))) ([v]x + (v v^T - vv I)); g = 1 + x[6] (1 without scale),
 *    finite and > 0 or DEGENERATE.  scale' = scale g; R' = dR R, each entry (a0 b0 + a1 b1) + a2 b2; t'_r = (g (dR (t - c))_r +
 *    c_r) + x[3 + r].
 *  9 metric 1, the loop: as f-17 rule 6 without the fixed-point stop: FEW; k > 0 and within eps: converged 2; k == max_iters:
 *    converged 0; else the step.
 * 10 the batch: results[b] and row b of idx are byte-equal to the single call from inits[b]; n_init in 1..1024. */
typedef struct sfmhip_icp_opts {
  int32_t max_iters;     /* 50 */
  int32_t with_scale;    /* 0 rigid, 1 similarity */
  int32_t min_pairs;     /* 3 for metric 0; at least 6 (7 with scale) for metric 1 */
  int32_t metric;        /* 0 point-to-point, 1 point-to-plane */
  int32_t one_to_one;    /* 1: a target point keeps only its best source */
  int32_t normal_stride; /* 3 or 4 (what sfmhip_cloud_normals writes); default 4 */
  double max_dist;       /* as f-17 */
  double eps;            /* metric 0: as f-17, default 0.  metric 1: must be > 0 */
  double trim;           /* (0, 1]; 1: off.  The fraction of the surviving pairs that is kept */
} sfmhip_icp_opts;
typedef struct sfmhip_icp_result {
  sfmhip_transform T;
  int32_t iterations, pairs, converged, flags; /* as sfmhip_register_result; pairs = the kept ones */
  double mse;       /* mean (double)d2 over the kept pairs */
  double plane_mse; /* mean r^2 over the kept pairs (metric 1; NaN for metric 0) */
  double trim_d2;   /* the trim threshold tau of the last pair set (+inf with trim = 1) */
} sfmhip_icp_result;
void sfmhip_icp_default_opts(sfmhip_icp_opts* opts);
/* target_normals: host, one row of normal_stride floats per target point; NULL allowed for metric 0.  opts: NULL for the
 * defaults; init: NULL for the identity; idx: NULL or one entry per source point, the kept pairs under out->T */
int sfmhip_cloud_register_icp(sfmhip_cloud* target, sfmhip_cloud* source, const float* target_normals, const sfmhip_icp_opts* opts,
                              const sfmhip_transform* init, sfmhip_icp_result* out, int32_t* idx);
/* results: n_init entries; idx: NULL or n_init rows of one entry per source point */
int sfmhip_cloud_register_icp_batch(sfmhip_cloud* target, sfmhip_cloud* source, const float* target_normals, const sfmhip_icp_opts* opts,
                                    const sfmhip_transform* inits, int n_init, sfmhip_icp_result* results, int32_t* idx);
/* With sfmhip_set_timing on (zeros while it is off): host-clock ms of the last call of either entry with this target, summed
 * over its iterations -- search, rejectors, sums, update + the record's read -- and the iterations of its longest problem. */
int sfmhip_cloud_register_icp_last_timing(sfmhip_cloud* target, double ms4[4], int32_t* iterations);

/* ---- the second half of create_mesh: Poisson surface reconstruction (reference src/Sfm.cpp:1365-1381) ----
 * pcl::Poisson at depth 7 on the cloud and its flipped normals, as a screened Poisson solve on the same device-resident
 * cloud.  The rules (PCL 1.8.1 parity is UNPINNED -- PCL is absent and its solver is an adaptive octree):
 *   deviations: the grid is uniform at full depth (PCL: adaptive octree), the extraction is marching tetrahedra (PCL:
 *   marching cubes).  PCL setters with no counterpart: samplesPerNode, isoDivide, solverDivide, manifold,
 *   outputPolygons; confidence has no effect on unit normals.
 *   1. samples: the finite points whose normal is finite and non-zero; the others are skipped.  No usable sample: an
 *      empty mesh, status OK.  depth 1..8 (7), scale 1..16 (1.1), point_weight >= 0 (4), cg_rtol in [0, 1) (1e-8),
 *      cg_max_iter (0 = 4 * 2^depth); outside: SFMHIP_ERR_ARG.
 *   2. cube: centre = midpoint of the samples' box (f64), side = scale * largest extent (extent 0: side 1),
 *      N = 2^depth cells per side, h = side / N, unknowns at the cell centres, u = (p - origin) / h - 1/2.
 *   3. splat: B(t) = 3/4 - t^2 (|t| < 1/2), (3/2 - |t|)^2 / 2 (|t| < 3/2), 0; V_c = sum B(u_p - c) n_p and
 *      W_c = sum B(u_p - c) over the samples of the 27 cells around c, in f64, gathered per cell (no atomics):
 *      neighbour cells ascending in (z, y, x), samples ascending by input index.  Nothing lands outside the cube.
 *   4. system: (L + point_weight diag(W)) chi = -div V in h = 1 units; L the 7-point negative Laplacian with chi = 0
 *      outside, div by central differences with V = 0 outside.
 *   5. conjugate gradients in f64 from chi = 0 until |r|^2 <= cg_rtol^2 |b|^2 or cg_max_iter steps; dot products in
 *      the fixed order of csrc/poisson.h (bricks of 16 x 4 x 4 cells, a 256-entry tree per brick, then the bricks by
 *      residue class mod 256 and the same tree); no contraction.  The decision is taken on the device.
 *   6. iso-value: the mean of the trilinear chi at the samples, summed in the same fixed order.
 *   7. extraction on the (N - 1)^3 cubes between cell centres, each split into the six tetrahedra around its main
 *      diagonal; a corner is inside iff chi < iso; one vertex per crossed edge at linear interpolation, id from (lower
 *      corner, edge class 0..6); triangles wound so that their normals point towards chi > iso.  Vertices ascending
 *      by edge id, triangles by (cube, tetrahedron, case order).  float32 xyz in cloud coordinates, int32 x 3.
 * normals: n rows of normal_stride floats, nx ny nz first -- 4 is the layout sfmhip_cloud_normals writes (the curvature
 * in the fourth float is not read), 3 is packed.
 * Hitting cg_max_iter is not an error: compare cg_iterations and cg_relative_residual of the summary with the options.
 * The default cap does not reach cg_rtol 1e-8 at depth 7 (about 6 * 2^depth steps are needed); create_mesh passes
 * 8 * 2^depth.  The handle keeps the call's device blocks (over 300 MB at depth 7) for its next call until it is
 * destroyed. */
typedef struct {
  int32_t depth;
  double scale, point_weight, cg_rtol;
  int32_t cg_max_iter;   /* 0: 4 * 2^depth */
  int32_t normal_stride; /* 3 or 4 (default) */
} sfmhip_poisson_opts;

typedef struct {
  int32_t n_samples, n_vertices, n_triangles, cg_iterations;
  double cg_relative_residual; /* |r| / |b| when the solve stopped */
  double iso_value;
  double origin[3], cell; /* the cube's low corner and h */
  int32_t grid;           /* N */
} sfmhip_poisson_summary;

typedef struct sfmhip_mesh sfmhip_mesh;
void sfmhip_poisson_default_opts(sfmhip_poisson_opts* opts);
int sfmhip_cloud_poisson(sfmhip_cloud* cloud, const float* normals, const sfmhip_poisson_opts* opts, sfmhip_mesh** out,
                         sfmhip_poisson_summary* summary);
int sfmhip_mesh_counts(const sfmhip_mesh* mesh, int32_t* n_vertices, int32_t* n_triangles);
int sfmhip_mesh_download(const sfmhip_mesh* mesh, float* vertices /* 3 nv */, int32_t* triangles /* 3 nt */);
void sfmhip_mesh_destroy(sfmhip_mesh* mesh);
/* staged: rules 1-4.  V: 3 N^3 (axis-major, cells x-fastest), W and rhs: N^3. */
int sfmhip_cloud_poisson_splat(sfmhip_cloud* cloud, const float* normals, const sfmhip_poisson_opts* opts, double* V, double* W,
                               double* rhs, sfmhip_poisson_summary* summary);
/* staged: rule 5 from a given right-hand side.  rr_bb (may be NULL): the final and the initial squared residual. */
int sfmhip_poisson_solve(sfmhip_ctx* ctx, int depth, const double* rhs, const double* W, double point_weight, double cg_rtol,
                         int cg_max_iter, double* chi, int32_t* iterations, double* rr_bb);
/* staged: rule 7 from a given field on an n^3 grid (any n in 2..256), grid point (x, y, z) at origin + (x + 1/2) cell. */
int sfmhip_poisson_extract(sfmhip_ctx* ctx, int n, const double* chi, double iso, const double* origin /* 3 */, double cell,
                           sfmhip_mesh** out);
/* host-clock ms of the last sfmhip_cloud_poisson call on this handle: samples + splat, solve, iso-value + extraction,
 * the whole call. */
int sfmhip_cloud_poisson_last_timing(sfmhip_cloud* cloud, double* ms4);

/* ---- finishing a mesh against the cloud it was made from (the reference has no mesh post-processing) ----
 * A Poisson surface is closed: over every hole in the data it invents a sheet.  The call trims what no point supports, drops
 * small components, and gives every vertex a colour, a normal and its nearest point.  The mesh stays a host object: the call
 * uploads the input mesh and downloads the output.  The rules (arithmetic: csrc/mesh.h, -ffp-contract=off, the device equal
 * to the g++ build bit for bit):
 *   M1. inputs: a vertex with a non-finite coordinate is never supported, whatever min_support says.  A triangle with a
 *       repeated index, or with an unsupported vertex, does not survive.  A cloud without a finite point or a mesh without a
 *       vertex: status OK and an empty output, every input vertex counted unsupported and every triangle trimmed.
 *   M2. support of vertex v over the finite cloud points p: d2 = the family's float dist2 (((dx dx) + dy dy) + dz dz); a
 *       point counts iff d2 < (float)(r * r), r squared in f64 -- sfmhip_cloud_radius_count's test, strict.  support = the
 *       count, not capped.  nearest / nearest_d2 = the least (d2, index) among the counted points (d2, then index); with none
 *       -1 and +inf.  Colour weights in f64: w = (1 - d2 / r2)^2 with r2 = (double)(float)(r * r); sw, sr, sg, sb summed in
 *       one order, that of the handle's radius grid for r (cells of r (1 + 1/1024), doubled while the grid exceeds 2^22
 *       cells, as sfmhip_cloud_radius_count and sfmhip_cloud_mls share it): ascending (cell id, input index), cell ids
 *       x-fastest.  A channel is (int)(s / sw + 0.5) clamped to 0..255; support 0 gives colour 0.  A vertex outside the
 *       cloud's box is looked up from the border cell it is clamped into: the block of cells around that cell still holds
 *       every point within r, and the distance test decides.
 *   M3. trim: a vertex is supported iff it is finite and support >= min_support; a triangle survives iff it has no repeated
 *       index and its three vertices are supported.
 *   M4. components: the vertices of the surviving triangles joined (a-b, b-c); a component's id is its least vertex index,
 *       its size its number of surviving triangles.  Components with size < min_component_triangles are dropped; with
 *       keep_largest = k > 0 only the first k by (size descending, id ascending) stay.  Integer atomics only, none whose
 *       order matters.
 *   M5. compaction: surviving triangles keep input order; the vertices at least one of them uses keep input order and are
 *       renumbered; vertex_src / triangle_src map output rows to input rows.
 *   M6. normals: per output vertex the f64 sum, over its output triangles ascending by output triangle index, of
 *       cross(b - a, c - a) of the widened floats (area-weighted, oriented as the triangles are), normalised in f64 and
 *       cast to float; a zero or non-finite length writes 0x7FC00000 three times.
 *   M7. area = sum of |cross| / 2 and volume = sum of a . (b x c) / 6 over the output triangles in f64: consecutive blocks
 *       of 256 triangles by the 256-slot tree of f-9, the block partials added in ascending order.  volume is a plain
 *       signed sum: a volume only for a closed mesh (no closedness test).
 * support_radius has no default: 0, negative or non-finite is SFMHIP_ERR_ARG, as a negative count is.  min_support 0 trims
 * nothing finite (the search still runs: counts, nearest, colours).  sfmhip_mesh_create wraps caller arrays (nv = 0 and
 * nt = 0 are accepted; a triangle index outside [0, nv) is SFMHIP_ERR_ARG).  A mesh that did not come out of
 * sfmhip_cloud_mesh_finish has no attributes: sfmhip_mesh_attributes on it is SFMHIP_ERR_STATE when any array is asked for;
 * rgb is filled only when the finishing call was given colours.  sfmhip_mesh_counts, sfmhip_mesh_download and
 * sfmhip_mesh_destroy serve every mesh.  The handle keeps the call's device blocks: a repeat call allocates nothing. */
typedef struct {
  double  support_radius;          /* cloud units; > 0 and finite, else SFMHIP_ERR_ARG: there is no default */
  int32_t min_support;             /* >= 0; 0: no trimming (the search still runs: counts, nearest, colours) */
  int32_t min_component_triangles; /* >= 0; components with fewer surviving triangles are dropped; 0: off */
  int32_t keep_largest;            /* >= 0; k > 0: only the k largest components survive; 0: off */
  int32_t reserved;
} sfmhip_mesh_finish_opts;
typedef struct {
  int32_t n_vertices_in, n_triangles_in, n_vertices, n_triangles;
  int32_t n_unsupported_vertices, n_trimmed_triangles; /* by M3 */
  int32_t n_components, n_components_kept;             /* after M3 / after M4 */
  double  area, volume;                                /* M7, of the output */
} sfmhip_mesh_finish_summary;
void sfmhip_mesh_finish_default_opts(sfmhip_mesh_finish_opts* opts); /* radius 0 (must be set), min_support 1, rest 0 */
int sfmhip_mesh_create(const float* vertices, int nv, const int32_t* triangles, int nt, sfmhip_mesh** out);
int sfmhip_cloud_mesh_finish(sfmhip_cloud* cloud, const uint32_t* rgb /* n, 0x00RRGGBB, or NULL */, const sfmhip_mesh* in,
                             const sfmhip_mesh_finish_opts* opts, sfmhip_mesh** out, sfmhip_mesh_finish_summary* summary);
/* each array may be NULL: normals 3 nv, rgb nv, support nv, nearest nv, nearest_d2 nv, vertex_src nv, triangle_src nt */
int sfmhip_mesh_attributes(const sfmhip_mesh* mesh, float* normals, uint32_t* rgb, int32_t* support, int32_t* nearest,
                           float* nearest_d2, int32_t* vertex_src, int32_t* triangle_src);
/* host-clock ms of the last sfmhip_cloud_mesh_finish call on this handle (timing on): search, trim + components, compaction +
 * normals + sums + download, the whole call; the call less the three stages is the upload of the mesh and the colours. */
int sfmhip_cloud_mesh_last_timing(sfmhip_cloud* cloud, double ms4[4]);

/* ---- adjustBundle solver core (reference src/BundleAdjustment.cpp:46-175) ---- */
typedef struct {
  int max_iterations;           /* 500   src/BundleAdjustment.cpp:118 */
  double max_time_s;            /* 10    src/BundleAdjustment.cpp:120 ; <=0 disables */
  double function_tolerance;    /* 1e-6  Ceres 1.13 defaults from here on */
  double gradient_tolerance;    /* 1e-10 */
  double parameter_tolerance;   /* 1e-8  */
  double initial_radius;        /* 1e4   */
  double max_radius;            /* 1e16  */
  double min_radius;            /* 1e-32 */
  double min_relative_decrease; /* 1e-3  */
  double min_lm_diagonal;       /* 1e-6  */
  double max_lm_diagonal;       /* 1e32  */
  int jacobi_scaling;           /* 1     */
  int max_consecutive_invalid;  /* 5     */
  int verbose;
} sfmhip_ba_opts;

enum { SFMHIP_BA_CONVERGENCE = 0, SFMHIP_BA_NO_CONVERGENCE = 1, SFMHIP_BA_FAILURE = 2 };

typedef struct {
  int termination; /* SFMHIP_BA_*; the C++ wrapper writes results back only on CONVERGENCE
                      (src/BundleAdjustment.cpp:126-129) */
  int iterations;
  int successful_steps;
  double initial_cost;
  double final_cost;
  double final_radius;
  double gradient_max_norm;
  double time_s;
  int spin_timeouts; /* reduced solves whose hand-off between fronts timed out (a busy device) and were repeated level by level;
                        0 in every run this build has measured.  They never change the LM trajectory. */
} sfmhip_ba_summary;

void sfmhip_ba_default_opts(sfmhip_ba_opts* o);

/* One-shot: host buffers in, optimised parameters out (in place).  cams6: n_cam x
 * (angle-axis 3, translation 3); pts3: n_pt x 3; one shared focal; one residual block per
 * (obs_cam[o], obs_pt[o], obs_xy[2o..2o+1]) with the principal point already subtracted. */
int sfmhip_ba_solve(sfmhip_ctx* ctx, int n_cam, int n_pt, int n_obs, double* cams6, double* pts3,
                    double* focal, const int32_t* obs_cam, const int32_t* obs_pt,
                    const double* obs_xy, const sfmhip_ba_opts* opts, sfmhip_ba_summary* summary);

/* Where the last sfmhip_ba_solve call on this context spent its time (milliseconds of host wall clock, stage by stage), and
 * whether it reused the problem the call before it had set up.  The one-shot entry point is what
 * BundleAdjustment::adjustBundle (reference include/BundleAdjustment.h:19-20, src/BundleAdjustment.cpp:46-123) maps to: the
 * reference builds its ceres::Problem from the containers on every call, and so does this -- create_ms is that cost --
 * unless the observation structure (n_cam, n_pt, obs_cam[], obs_pt[]) equals the previous call's, in which case the kept
 * problem takes the new measurements and parameters and create_ms is the comparison + the re-upload. */
typedef struct sfmhip_ba_solve_profile {
  double create_ms;     /* sfmhip_ba_create (or, plan_reused: structure comparison + new measurements) */
  double set_params_ms; /* parameters to the device */
  double run_ms;        /* the LM loop (the first call on a structure also plans the reduced system's front tree here) */
  double get_params_ms; /* parameters back */
  double keep_ms;       /* keeping the problem for the next call (a copy of obs_cam / obs_pt) or destroying it */
  double total_ms;
  int plan_reused;
  int front_plan_reused; /* a NEW structure whose camera graph equals the last one's: the front tree was not planned again */
} sfmhip_ba_solve_profile;
int sfmhip_ba_last_solve_profile(sfmhip_ctx* ctx, sfmhip_ba_solve_profile* out);
/* The library's host threads (a pool of up to 16 that lives as long as the process: the set-up's passes run on it) for a
 * caller's own pass over its containers -- fn(lo, hi, user) on disjoint blocks of [0, n), the calling thread taking one of
 * them; returns when all are done.  Below 20 000 items, or when the pool is busy, fn(0, n, user) runs on the caller alone /
 * on threads started for the call.  fn may call back into the library: a pass it starts runs on threads of its own.  What
 * BundleAdjustment::adjustBundle's mirror packs and writes back with (the reference walks its std::map tracks on one thread,
 * src/BundleAdjustment.cpp:83-110: 8 ms at cfg4). */
int sfmhip_host_parallel_for(int n, void (*fn)(int lo, int hi, void* user), void* user);

/* Persistent problem object (multi-GPU: every rank holds all cameras + focal and its own
 * block of points with their observations; the per-iteration sum of the reduced camera
 * system goes through `allreduce`, e.g. RCCL via torch.distributed). */
typedef int (*sfmhip_allreduce_fn)(void* device_f64_buffer, size_t count, void* user);

int sfmhip_ba_create(sfmhip_ctx* ctx, int n_cam, int n_pt, int n_obs, const int32_t* obs_cam,
                     const int32_t* obs_pt, const double* obs_xy, sfmhip_ba** out);
/* rank/world of the calling process; world==1 (the default) never calls fn.  The callback sums
 * `count` doubles in place across ranks (ncclAllReduce(sum, ncclDouble) over xGMI) and must be
 * ordered after the work already enqueued on the context's stream. */
int sfmhip_ba_set_allreduce(sfmhip_ba* ba, sfmhip_allreduce_fn fn, void* user, int rank, int world);
int sfmhip_ba_set_params(sfmhip_ba* ba, const double* cams6, const double* pts3, double focal);
int sfmhip_ba_get_params(sfmhip_ba* ba, double* cams6, double* pts3, double* focal);
int sfmhip_ba_run(sfmhip_ba* ba, const sfmhip_ba_opts* opts, sfmhip_ba_summary* summary);
/* `iters` LM iterations (linearise + Schur eliminate + all-reduce + reduced solve +
 * back-substitute + candidate cost, accept/reject as usual) without convergence tests.
 * Resumable: the first call after set_params linearises and computes the Jacobi scaling,
 * later calls continue the same trust-region state. */
int sfmhip_ba_iterate(sfmhip_ba* ba, int iters, sfmhip_ba_summary* summary);
/* One linearisation at the current parameters: reduced system of this rank's points,
 * dim = 6*n_cam+1, S row-major full symmetric, before any all-reduce.  Test hook. */
int sfmhip_ba_reduced_system(sfmhip_ba* ba, double radius, double* S, double* g, double* cost);
/* Residual and Jacobian of n single observations as the solver linearises them (SimpleReprojectionError,
 * reference src/BundleAdjustment.cpp:10-35; analytic derivative of the theta^2 branch autodiff takes).
 * cams6: n x 6, pts3: n x 3, obs_xy: n x 2; r: n x 2, Jc: n x (2x6 row-major), Jp: n x (2x3), Jf: n x 2.
 * Test hook. */
int sfmhip_ba_linearize_obs(sfmhip_ctx* ctx, int n, const double* cams6, const double* pts3, double focal,
                            const double* obs_xy, double* r, double* Jc, double* Jp, double* Jf);
/* Test hook: the solution z of the damped reduced system (S + D/radius) z = g at the current parameters, as the
 * solver's own factorisation (dense or dissected, see sfmhip_ba_reduced_layout) computes it; z: 6*n_cam + 1
 * doubles in the solver's scaled coordinates (the system sfmhip_ba_reduced_system returns); *chol_failed != 0 when
 * a pivot was not positive.  Single rank only. */
int sfmhip_ba_reduced_step(sfmhip_ba* ba, double radius, double* z, int* chol_failed);
/* How the reduced camera system of this problem is factored (decided at the first run / iterate; zeros before):
 * layout[0] = independent interior chains of the dissected camera graph (0: one dense factorisation),
 * layout[1] = 32-column tiles of the longest chain, layout[2] = tiles of the separator (with the focal),
 * layout[3] = tiles of the dense matrix.  The factorisation's dependency chain is layout[1] + layout[2] tiles
 * instead of layout[3].  Replaces nothing in the reference (Eigen's dense LLT, src/BundleAdjustment.cpp:116,
 * has no such choice); SFMHIP_BA_ND=0 in the environment keeps the dense factorisation. */
int sfmhip_ba_reduced_layout(sfmhip_ba* ba, int32_t layout[4]);
/* The front tree, when the camera graph dissects recursively into fronts that fit one compute unit each (the default
 * where it exists; SFMHIP_BA_ND=1 keeps the chains + separator plan, =0 the dense factorisation, =2 tree or dense):
 * tree[0] = fronts (0: no tree), tree[1] = levels, tree[2] = 32-column tile steps on the longest leaf-to-root path (the
 * dependency chain), tree[3] = tiles (own + border) of the largest front.  sfmhip_ba_reduced_layout then reports no
 * chains.  Behind Eigen's LLT, reference src/BundleAdjustment.cpp:116. */
int sfmhip_ba_reduced_tree(sfmhip_ba* ba, int32_t tree[4]);
/* Test hook: ONE trust-region decision (TrustRegionMinimizer + LevenbergMarquardtStrategy of Ceres 1.13 behind reference
 * src/BundleAdjustment.cpp:115-123), taken on the HOST by the very function the device runs at the end of every step evaluation
 * (lm_decide in csrc/ba.hip; compiled without contraction on both sides, so the two agree bit for bit).  Needs no GPU.
 * state: options in, trust-region state in and out; `accepted` is set when this decision took the candidate; `stop` is -1 while
 * the loop runs, an SFMHIP_BA_* termination type once a rule has fired (further calls change nothing), 100 when `solve_info` < 0
 * (a bounded spin ran out: neither an iteration nor a step). */
typedef struct {
  double gradient_tolerance, parameter_tolerance, function_tolerance, min_relative_decrease, max_radius, min_radius;
  int max_consecutive_invalid, max_iterations, timing_only /* sfmhip_ba_iterate: no convergence tests */, pad;
  double radius, decrease_factor, cost, gradient_max_norm, x_norm;
  int iterations, successful_steps, invalid_steps, lin_unread /* the last accepted step's linearisation has not been read */;
  int accepted, stop;
} sfmhip_lm_state;
typedef struct {
  double lin_cost, lin_failed_blocks, lin_gradient_max;                          /* of the linearisation at x */
  double candidate_cost, model_cost_change, step_norm2, candidate_norm2;         /* of the step evaluation */
  int solve_info, pad;                                                           /* > 0: a pivot was not positive; < 0: time-out */
} sfmhip_lm_inputs;
int sfmhip_ba_lm_decide(sfmhip_lm_state* state, const sfmhip_lm_inputs* in);
/* device seconds of the last run/iterate by kernel group:
 * [0]=linearise+eliminate [1]=allreduce [2]=reduced solve [3]=back-substitute+cost */
int sfmhip_ba_last_timing(sfmhip_ba* ba, double seconds[4], int* launches);
void sfmhip_ba_destroy(sfmhip_ba* ba);

/* ---- Dense multi-view stereo: map3D step 7 (reference src/Sfm.cpp:62-67 shells out to pmvs2) ----
 * Plane-sweep depth maps per reference view, then cross-view consistency fusion into one coloured, oriented cloud.
 * Parity with pmvs2 is UNPINNED (it expands patches; its output is not comparable point for point); the contract is
 * this rule list, whose arithmetic is csrc/mvs.h (compiled by g++ and hipcc; the device equals the host build bit for bit).
 *  1 images: one 8-bit gray image per view (+ optional BGR), one size, one K, [R|t] per view (x_cam = R X + t, 12 doubles
 *    row-major).  `level` L halves L times with the 2x2 box mean (a+b+c+d+2)>>2, an odd last row / column dropped;
 *    fx, fy halve, cx' = (cx + 0.5) / 2 - 0.5 (cy likewise).
 *  2 hypotheses: n_planes fronto-parallel planes of the reference view, uniform in inverse depth, index 0 at dmax and
 *    n_planes - 1 at dmin; per plane and source the host forms the 3x3 homography reference pixel -> source pixel in f64.
 *  3 sample: three f64 dot products (h0 x + h1 y) + h2 and two divisions, floor, fractions quantised to 1/32 round half up
 *    (32 carries), integer bilinear blend rounded to a 12-bit sample (8.4 fixed point, 0 ... 4080); invalid unless all four
 *    taps are inside the image and the point is in front of the source; the reference pixel's sample is 16 I.
 *  4 score: window (2 window + 1)^2 inside the reference image; integer sums N, r, r^2, q, q^2, rq (u32, window <= 7);
 *    NCC = (N rq - r q) / sqrt((N r^2 - (r)^2)(N q^2 - (q)^2)), terms in i64, one f64 product, sqrt and division.  A source
 *    counts if all its window samples are valid and its variance term is > 0; a reference pixel whose own variance term is
 *    0 or below var_min has no depth; a hypothesis scores the mean of its n_best largest NCCs (summed in descending order)
 *    and is invalid with fewer than n_best sources.
 *  5 winner: largest score, lowest index on ties, accepted if >= ncc_min; three-point parabola refinement in inverse depth
 *    when the winner is interior and both neighbours are valid.  Outputs: index (-1: none), depth (f32, 0: none), score.
 *  6 sources (sfmhip_mvs_run): the n_src other views with the nearest camera centres, ties by lower index.
 *  7 fusion: lift pixel p of view r at depth z to X; view v is consistent if X projects (rounded to the nearest pixel) onto a
 *    pixel with depth zv, |zv - z_in_v| <= eps z_in_v; keep X if 1 + consistent views >= min_views and r is the lowest view
 *    among itself and the consistent ones; order view, row, column; normal = unit vector from X to the centre of r; colour
 *    0x00RRGGBB from the level-L BGR image (gray replicated without one). */
typedef struct sfmhip_mvs sfmhip_mvs;
typedef struct sfmhip_mvs_opts {
  int32_t n_planes;  /* 128; 3 ... 256 */
  int32_t window;    /* 3; 1 ... 7 */
  int32_t n_src;     /* 4; 1 ... 8 */
  int32_t n_best;    /* 2; 1 ... 4 */
  int32_t min_views; /* 3 (the host mirror passes the reference's minImageNum 5) */
  int32_t pad;
  double ncc_min;    /* 0.7 */
  double eps;        /* 0.01 */
  double var_min;    /* 614656 = 49^2 16^2: gray values of standard deviation 1 at window 3, in 12-bit units */
} sfmhip_mvs_opts;
void sfmhip_mvs_default_opts(sfmhip_mvs_opts* opts);
/* gray[v]: rows x cols bytes; bgr: NULL or n_views pointers to rows x cols x 3.  SFMHIP_ERR_ARG: n_views < 2, a size of 0
 * (also after `level` halvings), a null image. */
int sfmhip_mvs_create(sfmhip_ctx* ctx, int n_views, int rows, int cols, const uint8_t* const* gray, const uint8_t* const* bgr,
                      const double* K9, const double* poses12, int level, sfmhip_mvs** out);
void sfmhip_mvs_destroy(sfmhip_mvs* h);
/* The working level: its size and K; with view >= 0 also that view's gray (and BGR) image.  Every output is nullable. */
int sfmhip_mvs_level(sfmhip_mvs* h, int32_t* rows, int32_t* cols, double* K9, int view, uint8_t* gray, uint8_t* bgr);
/* Rules 2-5 for one reference view against the given sources; the depth map stays on the handle for the fusion.  idx, depth,
 * score: rows x cols of the working level, nullable.  SFMHIP_ERR_ARG: dmin >= dmax or <= 0, options out of range, ref among
 * the sources, a source twice or out of range. */
int sfmhip_mvs_depthmap(sfmhip_mvs* h, int ref, int n_src, const int32_t* src, double dmin, double dmax, const sfmhip_mvs_opts* opts,
                        int32_t* idx, float* depth, float* score);
/* Test hook: a hand-made depth map for one view (0 = no depth). */
int sfmhip_mvs_set_depthmap(sfmhip_mvs* h, int view, const float* depth);
/* Rule 7 over the depth maps the handle holds (a view without one contributes nothing). */
int sfmhip_mvs_fuse(sfmhip_mvs* h, const sfmhip_mvs_opts* opts, int32_t* n_points);
/* Rule 6, every view's depth map between dmin[v] and dmax[v], then the fusion. */
int sfmhip_mvs_run(sfmhip_mvs* h, const double* dmin, const double* dmax, const sfmhip_mvs_opts* opts, int32_t* n_points);
/* The last fusion's points: xyz and normals 3 floats each, rgb one word each; nullable. */
int sfmhip_mvs_download(const sfmhip_mvs* h, float* xyz, float* normals, uint32_t* rgb);
/* ms of the last sfmhip_mvs_run / sfmhip_mvs_fuse: depth maps, fusion, whole call.  The depth maps are timed apart only under
 * sfmhip_set_timing (one more stream synchronisation); without it [0] is 0 and [1] holds both. */
int sfmhip_mvs_last_timing(const sfmhip_mvs* h, double ms3[3]);

/* ---- Lens distortion in front of the dense stereo: undistort the views ----
 * The plane sweep warps with pinhole homographies, so pictures from a lens with distortion (k1 k2 p1 p2 k3, the five
 * coefficients of the calibration file, as sfmhip_triangulate and sfmhip_pnp_ransac take them) are resampled once into the
 * pinhole camera of the SAME K.  The reference hands pmvs2 the raw pictures; there is no library here to pin parity against:
 * the contract is this rule list, whose arithmetic is csrc/undistort.h (compiled by g++ and hipcc; the device equals the host
 * build bit for bit).
 *  1 map: for destination pixel (x, y): xn = (x - cx) / fx, yn = (y - cy) / fy; the forward model of the projection
 *    (csrc/camera.h project_point: r2, r4, r6, a1, a2, a3, cdist, xd, yd in that order, f64); u = xd fx + cx, v = yd fy + cy.
 *    It depends on K, the coefficients and the size only: one map per call, shared by every view and channel.
 *  2 quantise: fu = floor(u), wx = floor((u - fu) 32 + 0.5); wx = 32 carries (wx = 0, ix + 1); v likewise.  floor is taken
 *    on the f64 value, negatives included (u = -1e-15 carries to ix = 0, wx = 0).
 *  3 validity, after the carry: a tap of weight zero is not read; the pixel is valid iff every tap of non-zero weight lies
 *    inside the source; a non-finite u or v is invalid.
 *  4 blend: ((a (32 - wx) + b wx)(32 - wy) + (c (32 - wx) + d wx) wy + 512) >> 10 per channel, 8 bit; an invalid pixel is 0 in
 *    every channel and 0 in the validity byte (1 otherwise).
 *  5 hence all-zero coefficients give the input byte for byte, every pixel valid, for any K.
 *  6 level masks: a pixel of level L is valid iff all 2^L x 2^L level-0 pixels under it are (a dropped odd row or column is
 *    simply absent).
 *  7 no depth at the seam: on a handle created with distortion, a reference pixel whose (2 window + 1)^2 window touches an
 *    invalid level-L pixel gets index -1, depth 0, score 0, applied after rules 2-5 of the stereo; the sweep and its sampling
 *    are untouched, so a black tap on the source side only lowers an NCC.
 * Known limit: K is kept, so pincushion coefficients leave invalid (black) margins and barrel coefficients crop the picture;
 * there is no new-camera-matrix or inscribed-rectangle step. */
/* Rules 1-5 for n_images pictures of one size: src[i], dst[i]: rows x cols x channels bytes (channels 1, or 3 interleaved);
 * valid: rows x cols bytes, nullable -- ONE mask, it is the same for every picture.  SFMHIP_ERR_ARG: a size or count of 0,
 * channels other than 1 or 3, a null pointer, fx or fy of 0, a non-finite K entry or coefficient. */
int sfmhip_image_undistort(sfmhip_ctx* ctx, int n_images, int rows, int cols, int channels, const uint8_t* const* src,
                           const double K9[9], const double dist5[5], uint8_t* const* dst, uint8_t* valid);
/* With sfmhip_set_timing on: the kernel time (ms, by events on the context's stream) of the last sfmhip_image_undistort call:
 * ms2 = map, gather. */
int sfmhip_image_undistort_last_timing(sfmhip_ctx* ctx, double ms2[2]);
/* sfmhip_mvs_create on pictures of a lens with distortion: gray and BGR are undistorted on the device (rules 1-5, one map),
 * then everything proceeds as in sfmhip_mvs_create with the same K; the handle keeps the level mask (rule 6) and
 * sfmhip_mvs_depthmap / sfmhip_mvs_run apply rule 7.  SFMHIP_ERR_ARG as sfmhip_mvs_create and sfmhip_image_undistort; *out is
 * null after a refusal. */
int sfmhip_mvs_create_distorted(sfmhip_ctx* ctx, int n_views, int rows, int cols, const uint8_t* const* gray,
                                const uint8_t* const* bgr, const double K9[9], const double dist5[5], const double* poses12, int level,
                                sfmhip_mvs** out);
/* The mask of the working level (rule 6), rows x cols bytes of sfmhip_mvs_level's size; all ones on a handle made by
 * sfmhip_mvs_create. */
int sfmhip_mvs_valid(sfmhip_mvs* h, uint8_t* valid);

/* ---- multi-view feature tracks and their N-view triangulation (PARITY UNPINNED: the reference links a point
 * to the two views it was triangulated from and never merges) ----
 * A handle holds, on the device, the tracks of one set of pair lists as the CSR sfmhip_find_2d3d takes.
 *   T1. A node is (image, feature), id = base[image] + feature, base = the exclusive scan of n_feat.  An edge is one match of
 *       one pair (match_q in the pair's first image, match_t in its second).  A match index < 0 or >= that image's n_feat, a
 *       pair that names an image outside [0, n_images) or the same image twice, a negative count or n_feat, or more than
 *       2^31 - 2 nodes or edges refuse the whole call with SFMHIP_ERR_ARG (the matches are checked on the device, by a flag,
 *       before anything is made; *out is not written).  Duplicate edges and duplicate pairs are allowed.
 *   T2. Components of that graph by a union-find whose roots only fall (atomicMin): a component's root is its least node id,
 *       whatever the order of the edges.
 *   T3. A component is conflicting when two of its nodes lie in one image.  (Nodes ascend by (image, feature); a stable sort
 *       by root leaves every component in that order, and a conflict is two neighbours of one image.)
 *   T4. A component is kept when it is not conflicting and has >= max(2, min_len) nodes.  A conflicting one is dropped whole.
 *   T5. Tracks are numbered by ascending root; inside a track the nodes ascend by (view, feature).  trk_ptr[n_tracks + 1],
 *       trk_view / trk_feat[n_obs], node_track[nodes] (-1: in no track).  The bytes depend on the edge SET alone.
 *   n_pairs = 0, counts all 0, images without features: SFMHIP_OK, 0 tracks.
 * stats: nodes; edges (with duplicates); components of >= 2 nodes; of those the conflicting ones; the non-conflicting ones
 * shorter than min_len; n_tracks; n_obs.
 * N-view triangulation of every track (sfmhip_tracks_triangulate):
 *   R1. The used observations of a track are those in views with has_pose != 0, ascending view; m of them.  m < 2: keep = 0,
 *       X = NaN.  err (n_obs, aligned with trk_view) is -1.0f at every unused observation.
 *   R2. Each used pixel goes through cv::undistortPoints' five iterations and gives the rows x P[2,:] - P[0,:] and
 *       y P[2,:] - P[1,:] (as sfmhip_triangulate forms them); X is the smallest right singular vector of the 2m x 4 system by
 *       OpenCV's one-sided Jacobi (sums over rows ascending, max(2m, 30) sweeps, descending selection sort, last row),
 *       divided by its fourth entry when that is not 0.
 *   R3. err = (float)sqrt(dx^2 + dy^2) of cv::projectPoints in every used view.
 *   R4. keep = m >= max(2, min_views) && !(any max_err < err), so a NaN error keeps its point as sfmhip_triangulate does; with
 *       front_only also P[2,:] (X, 1) > 0 in every used view.
 *   R5. A track with two used observations gives the bits sfmhip_triangulate gives for those two views.
 * poses: 12 doubles per image ([R|t], read only where has_pose); xy: pixel pairs, image v's feature f at
 * xy[2 (xy_ptr[v] + f)]; a posed view with fewer than n_feat[v] pixels, or a decreasing xy_ptr, is SFMHIP_ERR_ARG.  Every
 * output may be NULL: X 3 n_tracks, err n_obs, n_used and keep n_tracks. */
#define SFMHIP_TRACKS_STAGES 6
typedef struct sfmhip_tracks sfmhip_tracks;
typedef struct sfmhip_tracks_opts {
  int32_t min_len;     /* 2 */
  int32_t front_only;  /* 0: the reference has no cheirality test */
} sfmhip_tracks_opts;
typedef struct sfmhip_tracks_stats {
  int64_t nodes, edges, components, conflicting, short_tracks, n_tracks, n_obs;
} sfmhip_tracks_stats;
void sfmhip_tracks_default_opts(sfmhip_tracks_opts* opts);
/* host lists in sfmhip_matchplan_fetch's layout: counts[n_pairs], match_q / match_t packed pair after pair.  opts: NULL = defaults */
int sfmhip_tracks_build(sfmhip_ctx* ctx, int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts,
                        const int32_t* match_q, const int32_t* match_t, const sfmhip_tracks_opts* opts, sfmhip_tracks** out);
/* the lists of the plan's last run, read where they lie on the device; n_feat = the image set's row counts.  The same bytes as
 * sfmhip_tracks_build on the fetched lists. */
int sfmhip_tracks_build_from_plan(sfmhip_matchplan* plan, const sfmhip_tracks_opts* opts, sfmhip_tracks** out);
int sfmhip_tracks_counts(const sfmhip_tracks* tracks, sfmhip_tracks_stats* stats);
int sfmhip_tracks_download(const sfmhip_tracks* tracks, int32_t* trk_ptr, int32_t* trk_view, int32_t* trk_feat, int32_t* node_track);
int sfmhip_tracks_triangulate(sfmhip_tracks* tracks, const double* poses, const uint8_t* has_pose, const double K[9], const double dist[5],
                              const int32_t* xy_ptr, const double* xy, float max_err, int min_views, double* X, float* err,
                              int32_t* n_used, uint8_t* keep);
/* With sfmhip_set_timing on, seconds by events on the context's stream: check, hook + flatten, sort by root, numbering + CSR,
 * length buckets (the build), and the kernel of the last sfmhip_tracks_triangulate. */
int sfmhip_tracks_last_timing(const sfmhip_tracks* tracks, double seconds[SFMHIP_TRACKS_STAGES]);
void sfmhip_tracks_destroy(sfmhip_tracks* tracks);

/* ---- two-view verification of match lists before the tracks (PARITY UNPINNED, as for the score entries: the
 * reference hands its ratio-test lists on unfiltered) ----
 * A handle holds, on the device, one set of pair lists after the verification, in a match plan's layout (`stride` slots per
 * pair, entries in list order, counts[n_pairs]), so that the tracks builder reads it unchanged.
 *   V1. For pair p = (a, b), match i has the pixel of image a's feature match_q[i] on the left and of image b's feature
 *       match_t[i] on the right, in list order; image v's feature f at xy[2 (xy_ptr[v] + f)], as sfmhip_tracks_triangulate
 *       takes them.  Both are normalised as findEssentialMat does, x * (1 / fx) + (-cx * (1 / fx)) and likewise y, by the kernel
 *       that gathers them from the lists where they lie; no pixel is stored per match.  xy is uploaded once per call.
 *   V2. The model of a pair is sfmhip_score_essential's RANSAC, unchanged (sample streams per count, chunks, keep rule,
 *       iteration limit), started from the gathered points.  The host reads the n_pairs counts once.
 *   V3. The mask of a match: 0 without a model, 1 for every match of a pair of exactly five with a model, else the RANSAC's
 *       inlier test under the pair's best E -- the mask sfmhip_score_essential returns.
 *   V4. kept[p] = the pair has a model and inliers[p] >= min_inliers.  A pair that is not kept has output count 0; inliers,
 *       iterations and E (9 per pair, zero without a model) are reported for every pair.
 *   V5. A kept pair's output list is its matches with a non-zero mask in their input order; its count equals inliers[p].  The
 *       input lists are not written.
 *   V6. SFMHIP_ERR_ARG, *out not written: a match index < 0 or >= its image's n_feat, or a pair naming an image outside
 *       [0, n_images) or the same image twice (checked on the device, by a flag, before the RANSAC); a negative count or one
 *       above the stride; more than 2^31 - 2 matches; a negative xy_ptr[0], a decreasing xy_ptr, an image with
 *       xy_ptr[v + 1] - xy_ptr[v] < n_feat[v]; prob outside (0, 1); NULL K or xy_ptr; NULL xy with any match present.
 *       n_pairs = 0, counts all 0, pairs of fewer than five matches: SFMHIP_OK, an empty set.
 * sfmhip_score_last_flags(ctx) reports the five-point corner flags of the call, as for sfmhip_score_essential.
 * stats: pairs; of those the kept ones; those without a model; the matches given; the matches kept. */
typedef struct sfmhip_verified sfmhip_verified;
typedef struct sfmhip_verify_opts {
  double prob;         /* 0.999: findEssentialMat's, as findBestPair calls it */
  double threshold;    /* 1.0 px */
  int32_t min_inliers; /* 15: a pair with fewer RANSAC inliers keeps no match (policy, the caller's to change) */
  int32_t reserved;
} sfmhip_verify_opts;
typedef struct sfmhip_verify_stats {
  int64_t pairs, pairs_kept, pairs_no_model, matches_in, matches_out;
} sfmhip_verify_stats;
void sfmhip_verify_default_opts(sfmhip_verify_opts* opts);
/* the lists of the plan's last run, read where they lie on the device; n_feat = the image set's row counts.  opts: NULL = defaults */
int sfmhip_matchplan_verify(sfmhip_matchplan* plan, const int32_t* xy_ptr, const double* xy, const double K[9],
                            const sfmhip_verify_opts* opts, sfmhip_verified** out);
/* host lists in sfmhip_matchplan_fetch's layout.  The same bytes as sfmhip_matchplan_verify on a plan that holds them. */
int sfmhip_verify_lists(sfmhip_ctx* ctx, int n_images, const int32_t* n_feat, int n_pairs, const int32_t* pairs, const int32_t* counts,
                        const int32_t* match_q, const int32_t* match_t, const int32_t* xy_ptr, const double* xy, const double K[9],
                        const sfmhip_verify_opts* opts, sfmhip_verified** out);
int sfmhip_verified_counts(const sfmhip_verified* verified, sfmhip_verify_stats* stats);
/* Every output may be NULL: counts, inliers, iterations and kept n_pairs; match_q / match_t packed pair after pair
 * (stats.matches_out entries); E 9 n_pairs. */
int sfmhip_verified_download(const sfmhip_verified* verified, int32_t* counts, int32_t* match_q, int32_t* match_t, int32_t* inliers,
                             int32_t* iterations, double* E, uint8_t* kept);
/* the tracks of the verified lists, read where they lie on the device: the same bytes as sfmhip_tracks_build on the download */
int sfmhip_tracks_build_from_verified(const sfmhip_verified* verified, const sfmhip_tracks_opts* opts, sfmhip_tracks** out);
/* seconds of the call that made the handle, by the host's clock between its stream synchronisations: uploads + gather, the
 * RANSAC, the compaction, and the whole call */
int sfmhip_verified_last_timing(const sfmhip_verified* verified, double seconds[4]);
void sfmhip_verified_destroy(sfmhip_verified* verified);

#ifdef __cplusplus
}
#endif
#endif
