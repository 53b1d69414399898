// DendrometryE.h -- the reference's Dendrometry class (include/DendrometryE.h, src/DendrometryE.cpp:3-29) over
// sfmhip_cloud_minmax: pcl::getMinMax3D of the dense cloud and "Total Height" = cv::norm(max - min).  The numbers the
// call prints stay readable afterwards (the reference only prints them).  measure() / estimateTree() are what the
// reference leaves blank: sfmhip_cloud_dendro_profile on the cloud, or on one cluster of the segmentation.
#pragma once
#include <vector>
#include "pcllite.h"
#include "sfmhip.h"

class Dendrometry {
 private:
  float min_[3] = {0, 0, 0}, max_[3] = {0, 0, 0};
  double height_ = 0;
  sfmhip_dendro_result tree_ = {};
  std::vector<sfmhip_dendro_slice> profile_;

 public:
  Dendrometry() {}
  ~Dendrometry() {}

  void estimate(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL);

  const float* minPt() const { return min_; }
  const float* maxPt() const { return max_; }
  double totalHeight() const { return height_; }

  // the measurements of the points with labels[i] == label (labels == nullptr: of every finite point); opts == nullptr:
  // sfmhip_dendro_default_opts.  Returns the library's status.
  int measure(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_dendro_opts* opts = nullptr);
  // measure(), then the reference's printed block with every blank filled
  int estimateTree(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_dendro_opts* opts = nullptr);

  const sfmhip_dendro_result& tree() const { return tree_; }
  const std::vector<sfmhip_dendro_slice>& stemProfile() const { return profile_; }
  double treeHeight() const { return tree_.total_height; }
  double dbh() const { return tree_.dbh; }
  double crownBaseHeight() const { return tree_.crown_base_height; }
  double liveCrown() const { return tree_.live_crown; }
  double spreadNS() const { return tree_.spread_ns; }
  double spreadEW() const { return tree_.spread_ew; }
};
