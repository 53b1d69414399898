// DendrometryE.h -- the reference's Dendrometry class (include/DendrometryE.h, src/DendrometryE.cpp:3-29) over
// sfmhip_cloud_minmax: pcl::getMinMax3D of the dense cloud and "Total Height" = cv::norm(max - min).  The numbers the
// call prints stay readable afterwards (the reference only prints them).
#pragma once
#include "pcllite.h"

class Dendrometry {
 private:
  float min_[3] = {0, 0, 0}, max_[3] = {0, 0, 0};
  double height_ = 0;

 public:
  Dendrometry() {}
  ~Dendrometry() {}

  void estimate(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL);

  const float* minPt() const { return min_; }
  const float* maxPt() const { return max_; }
  double totalHeight() const { return height_; }
};
