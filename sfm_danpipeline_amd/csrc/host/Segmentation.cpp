// Segmentation.cpp -- Segmentation::color_based_growing_segmentation (reference src/Segmentation.cpp:3-66) in the host
// mirror: loadPCDFile, PassThrough on z in [0, 14] and RegionGrowingRGB with the reference's setters, on the device
// (sfmhip_cloud_passthrough, sfmhip_cloud_segment_rgb).  The printed lines are the reference's.
#include "Segmentation.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include "hip_backend.h"

namespace {

void check(int rc, const char* what) {
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] %s: %s\n", what, sfmhip_error_string(rc));
    std::abort();  // (no CPU fallback behind the drop-in)
  }
}

}  // namespace

int Segmentation::color_based_growing_segmentation() {
  clusters_.clear();
  labels_.clear();
  cloud_.reset(new pcl::PointCloud<pcl::PointXYZRGB>());
  pcl::io::loadPCDFile(input_, *cloud_);

  std::cout << "************************************************" << std::endl;
  std::cout << "    COLOR BASE GROWING SEGMENTATION             " << std::endl;
  std::cout << "************************************************" << std::endl;

  if (cloud_->size() <= 0) {
    std::cout << "Cloud reading failed. no data points found" << std::endl;
    return -1;
  }

  std::cout << "Preparing options for segmentation..." << std::endl;

  const int n = (int)cloud_->size();
  std::vector<float> xyz((size_t)3 * n);
  std::vector<uint32_t> rgb((size_t)n);
  for (int i = 0; i < n; ++i) {
    const pcl::PointXYZRGB& p = cloud_->points[i];
    xyz[3 * (size_t)i] = p.x;
    xyz[3 * (size_t)i + 1] = p.y;
    xyz[3 * (size_t)i + 2] = p.z;
    rgb[i] = p.rgba;
  }
  sfmhip_cloud* dev = nullptr;
  check(sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev), "sfmhip_cloud_create");
  std::vector<int32_t> indices((size_t)n + 1);
  int32_t n_idx = 0;
  check(sfmhip_cloud_passthrough(dev, 2, 0.0f, 14.0f, 0, indices.data(), &n_idx), "sfmhip_cloud_passthrough");

  sfmhip_segment_opts opts;
  sfmhip_segment_default_opts(&opts);  // setDistanceThreshold(10), setPointColorThreshold(6), setRegionColorThreshold(5), setMinClusterSize(600)

  std::cout << "Input cloud:" << cloud_->size() << "\n" << "Distance threshold:" << 10 << "\n"
            << "Point color threshold:" << 6 << "\n" << "Region color threshold:" << 5 << "\n"
            << "Clusters size:" << 600 << std::endl;

  std::cout << "Extracting clusters..." << std::endl;
  labels_.assign((size_t)n, -1);
  int32_t n_clusters = 0;
  if (n_idx > 0)  // (an empty index list: RegionGrowingRGB extracts nothing)
    check(sfmhip_cloud_segment_rgb(dev, rgb.data(), indices.data(), n_idx, &opts, labels_.data(), &n_clusters, nullptr),
          "sfmhip_cloud_segment_rgb");
  sfmhip_cloud_destroy(dev);
  clusters_.resize((size_t)n_clusters);
  for (int i = 0; i < n; ++i)
    if (labels_[i] >= 0) clusters_[labels_[i]].indices.push_back(i);
  if (clusters_.size() <= 0) {
    std::cerr << "Error: could not extract enough clusters." << std::endl;
    std::cout << "Extract:" << clusters_.size() << " clusters. Min=600" << std::endl;
    return -1;
  }
  std::cout << "Extract:" << clusters_.size() << " clusters" << std::endl;

  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
  return 0;
}
