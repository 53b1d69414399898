// Segmentation.h -- the reference's Segmentation class (include/Segmentation.h, src/Segmentation.cpp:3-66) over
// sfmhip_cloud_segment_rgb: pcl::RegionGrowingRGB on the indices of a PassThrough on z, with the reference's constants.
// Deviations: the call returns a status where the reference calls std::exit(-1); the viewer and getColoredCloud()'s
// random colours are not mirrored; the clusters stay readable afterwards; the PCD path can be set (default MAP3D.pcd in
// the working directory, the reference's literal).
#pragma once
#include <string>
#include <vector>
#include "pcllite.h"

class Segmentation {
 private:
  std::string input_ = "MAP3D.pcd";
  std::vector<pcl::PointIndices> clusters_;
  std::vector<int> labels_;
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud_;

 public:
  Segmentation() {}
  ~Segmentation() {}

  // 0: clusters extracted; -1: the cloud is empty or unreadable, or no cluster came out (where the reference exits)
  int color_based_growing_segmentation();

  void setInputFile(const std::string& path) { input_ = path; }
  // cluster c lists its points in ascending index (PCL's std::vector<pcl::PointIndices>)
  const std::vector<pcl::PointIndices>& clusters() const { return clusters_; }
  // per point of the loaded cloud: its cluster, -1 = in none
  const std::vector<int>& labels() const { return labels_; }
  // the cloud the call loaded (what main passes on to Dendrometry::estimate)
  pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloud() { return cloud_; }
};
