// DendrometryE.h -- the reference's Dendrometry class (include/DendrometryE.h, src/DendrometryE.cpp:3-29) over
// sfmhip_cloud_minmax: pcl::getMinMax3D of the dense cloud and "Total Height" = cv::norm(max - min).  The numbers the
// call prints stay readable afterwards (the reference only prints them).  measure() / estimateTree() are what the
// reference leaves blank: sfmhip_cloud_dendro_profile on the cloud, or on one cluster of the segmentation.
// findGround() is the vertical frame they need on a reconstruction's cloud: sfmhip_cloud_ground_plane;
// the overloads of measure() / estimateTree() that take ground options level first.  findTrees() cuts a levelled plot into
// trees: sfmhip_cloud_trees; estimatePlot() is the chain ground plane -> trees -> one measurement per tree.
// findTerrain() is the terrain model of a plot that undulates: sfmhip_cloud_terrain; the estimatePlot()
// overload that takes terrain options puts it, and the height normalisation, between the ground plane and the trees.
// findCrowns() finds the trees of a plot seen from above, by their crowns on the terrain's canopy raster: sfmhip_cloud_crowns
// (DESIGN.md f-21); the estimatePlot() overload that takes crown options uses it where the other uses the stems.
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
  sfmhip_ground_result ground_ = {};
  sfmhip_trees_result trees_ = {};
  std::vector<int> treeOf_;
  std::vector<sfmhip_tree_stem> stems_;
  std::vector<sfmhip_dendro_result> plot_;
  sfmhip_terrain_result terrain_ = {};
  std::vector<int> isGround_;
  std::vector<float> hag_;
  sfmhip_crowns_result crowns_ = {};
  std::vector<sfmhip_crown_top> tops_;
  // sfmhip_cloud_terrain on a handle made from cloudPCL; with `keep`, the handle is handed over instead of destroyed
  int terrainOn(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_terrain_opts& opts,
                sfmhip_cloud** keep);

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

  // the ground plane of the points with labels[i] == label (labels == nullptr: of every finite point); cam_centres: nullptr or
  // 3 n_cam doubles in the cloud's frame; opts == nullptr: sfmhip_ground_default_opts.  Returns the library's status.
  int findGround(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const double* cam_centres = nullptr,
                 int n_cam = 0, const sfmhip_ground_opts* opts = nullptr);
  // findGround() over every finite point, then measure() / estimateTree() on the cluster with up, north and ground taken
  // from it (opts' scale and the rest of its fields stay).  SFMHIP_ERR_ARG when no plane was found.
  int measure(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_ground_opts& ground_opts,
              const double* cam_centres, int n_cam, const sfmhip_dendro_opts* opts = nullptr);
  int estimateTree(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_ground_opts& ground_opts,
                   const double* cam_centres, int n_cam, const sfmhip_dendro_opts* opts = nullptr);
  const sfmhip_ground_result& ground() const { return ground_; }

  // the trees of the points with labels[i] == label (labels == nullptr: of every finite point): treeOf()[i] is point i's tree
  // or -1, stems() one row per tree.  opts must carry the frame and the ground (sfmhip_trees_opts_from_ground).
  int findTrees(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_trees_opts& opts);
  // findGround() over every finite point, findTrees() in its frame, then the measurement of every tree; prints one line per
  // tree in estimateTree()'s wording.  trees_opts / dendro_opts == nullptr: the defaults; their scale stays the caller's.
  // SFMHIP_ERR_ARG when no plane was found.
  int estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts, const double* cam_centres,
                   int n_cam, const sfmhip_trees_opts* trees_opts = nullptr, const sfmhip_dendro_opts* dendro_opts = nullptr);
  // the terrain model of the points with labels[i] == label (labels == nullptr: of every finite point) in the frame `opts`
  // carries (sfmhip_terrain_opts_from_ground): sfmhip_cloud_terrain.  isGround()[i] is 1 for a ground point,
  // heightAboveGround()[i] point i's height above the terrain in cloud units (NaN: none).
  int findTerrain(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_terrain_opts& opts);
  // estimatePlot() over a terrain: findGround(), the terrain in its frame, then the trees and one measurement per tree on the
  // normalised cloud (up +z, north +y, ground 0), which stays on the device; treeOf() indexes cloudPCL.
  int estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts, const double* cam_centres,
                   int n_cam, const sfmhip_terrain_opts& terrain_opts, const sfmhip_trees_opts* trees_opts = nullptr,
                   const sfmhip_dendro_opts* dendro_opts = nullptr);
  // the trees of a plot by their crowns: findTerrain() with `terrain_opts`, then sfmhip_cloud_crowns on its canopy raster
  // (DESIGN.md f-21).  treeOf()[i] is the tree of point i or -1, tops() one row per tree; no stem point is needed.
  int findCrowns(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_terrain_opts& terrain_opts, const sfmhip_crowns_opts& crown_opts);
  // estimatePlot() by crowns: findGround(), the terrain in its frame, the crowns on its canopy raster, then one measurement per
  // crown on the normalised cloud (up +z, north +y, ground 0), which stays on the device; treeOf() indexes cloudPCL.
  int estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts, const double* cam_centres,
                   int n_cam, const sfmhip_terrain_opts& terrain_opts, const sfmhip_crowns_opts& crown_opts,
                   const sfmhip_dendro_opts* dendro_opts = nullptr);
  const sfmhip_crowns_result& crowns() const { return crowns_; }
  const std::vector<sfmhip_crown_top>& tops() const { return tops_; }
  const sfmhip_terrain_result& terrain() const { return terrain_; }
  const std::vector<int>& isGround() const { return isGround_; }
  const std::vector<float>& heightAboveGround() const { return hag_; }
  const sfmhip_trees_result& trees() const { return trees_; }
  const std::vector<int>& treeOf() const { return treeOf_; }
  const std::vector<sfmhip_tree_stem>& stems() const { return stems_; }
  const std::vector<sfmhip_dendro_result>& plot() const { return plot_; }

  const sfmhip_dendro_result& tree() const { return tree_; }
  const std::vector<sfmhip_dendro_slice>& stemProfile() const { return profile_; }
  double treeHeight() const { return tree_.total_height; }
  double dbh() const { return tree_.dbh; }
  double crownBaseHeight() const { return tree_.crown_base_height; }
  double liveCrown() const { return tree_.live_crown; }
  double spreadNS() const { return tree_.spread_ns; }
  double spreadEW() const { return tree_.spread_ew; }
};
