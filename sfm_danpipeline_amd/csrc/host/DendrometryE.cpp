// DendrometryE.cpp -- Dendrometry::estimate (reference src/DendrometryE.cpp:3-29) in the host mirror: the bounds of the
// cloud on the device (sfmhip_cloud_minmax) and the reference's printed lines, the empty ones included; measure() and
// estimateTree() fill them (one sfmhip_cloud_dendro_profile call: the scalars and the stem table); findGround() and the
// levelling overloads put sfmhip_cloud_ground_plane in front of them; findTrees() and estimatePlot() put sfmhip_cloud_trees
// between the two, for a plot of several trees; findTerrain() and the estimatePlot() overload with terrain options put
// sfmhip_cloud_terrain and its normalised cloud, which never leaves the device, in front of the trees; findCrowns() and the
// estimatePlot() overload with crown options find the trees by sfmhip_cloud_crowns on the terrain's canopy raster instead.
#include "DendrometryE.h"
#include <cstdio>
#include <cstdlib>
#include <iostream>
#include <vector>
#include "hip_backend.h"

void Dendrometry::estimate(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL) {
  std::cout << "************************************************" << std::endl;
  std::cout << "              DENDROMETRY ESTIMATION            " << std::endl;
  std::cout << "************************************************" << std::endl;

  const int n = (int)cloudPCL->size();
  std::vector<float> xyz((size_t)3 * n + 3);
  for (int i = 0; i < n; ++i) {
    xyz[3 * (size_t)i] = cloudPCL->points[i].x;
    xyz[3 * (size_t)i + 1] = cloudPCL->points[i].y;
    xyz[3 * (size_t)i + 2] = cloudPCL->points[i].z;
  }
  sfmhip_cloud* dev = nullptr;
  int rc = sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev);
  if (rc == SFMHIP_OK) rc = sfmhip_cloud_minmax(dev, min_, max_, &height_);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_minmax: %s\n", sfmhip_error_string(rc));
    std::abort();  // (no CPU fallback behind the drop-in)
  }
  sfmhip_cloud_destroy(dev);

  std::cout << "Max: [" << max_[0] << ", " << max_[1] << ", " << max_[2] << "]" << std::endl;  // (cv::Point3f's operator<<)
  std::cout << "Min: [" << min_[0] << ", " << min_[1] << ", " << min_[2] << "]" << std::endl;

  std::cout << "*** Measurements ***" << std::endl;
  std::cout << "Total Height =" << height_ << std::endl;
  std::cout << "Altura copa viva=" << std::endl;
  std::cout << "Altura base de copa=" << std::endl;
  std::cout << "Altura DAP=" << 1.3 << std::endl;
  std::cout << "DAP=" << std::endl;
  std::cout << "Amplitud N-S=" << std::endl;
  std::cout << "Amplitud E-W=" << std::endl;

  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
}

int Dendrometry::measure(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_dendro_opts* opts) {
  sfmhip_dendro_opts o;
  if (opts)
    o = *opts;
  else
    sfmhip_dendro_default_opts(&o);
  const int n = (int)cloudPCL->size();
  std::vector<float> xyz((size_t)3 * n + 3);
  for (int i = 0; i < n; ++i) {
    xyz[3 * (size_t)i] = cloudPCL->points[i].x;
    xyz[3 * (size_t)i + 1] = cloudPCL->points[i].y;
    xyz[3 * (size_t)i + 2] = cloudPCL->points[i].z;
  }
  sfmhip_cloud* dev = nullptr;
  int rc = sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev);
  if (rc != SFMHIP_OK) return rc;
  int32_t S = 0;
  profile_.assign(4096, sfmhip_dendro_slice());
  rc = sfmhip_cloud_dendro_profile(dev, labels, label, &o, (int)profile_.size(), profile_.data(), &S, &tree_);
  profile_.resize(rc == SFMHIP_OK ? (size_t)S : 0);
  sfmhip_cloud_destroy(dev);
  return rc;
}

int Dendrometry::estimateTree(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_dendro_opts* opts) {
  const int rc = measure(cloudPCL, labels, label, opts);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_dendrometry: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  sfmhip_dendro_opts o;
  if (opts)
    o = *opts;
  else
    sfmhip_dendro_default_opts(&o);
  std::cout << "************************************************" << std::endl;
  std::cout << "              DENDROMETRY ESTIMATION            " << std::endl;
  std::cout << "************************************************" << std::endl;
  std::cout << "*** Measurements ***" << std::endl;
  std::cout << "Total Height =" << tree_.total_height << std::endl;
  std::cout << "Altura copa viva=" << tree_.live_crown << std::endl;
  std::cout << "Altura base de copa=" << tree_.crown_base_height << std::endl;
  std::cout << "Altura DAP=" << o.dbh_height << std::endl;
  std::cout << "DAP=" << tree_.dbh << std::endl;
  std::cout << "Amplitud N-S=" << tree_.spread_ns << std::endl;
  std::cout << "Amplitud E-W=" << tree_.spread_ew << std::endl;
  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
  return rc;
}

int Dendrometry::findGround(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const double* cam_centres,
                            int n_cam, const sfmhip_ground_opts* opts) {
  sfmhip_ground_opts o;
  if (opts)
    o = *opts;
  else
    sfmhip_ground_default_opts(&o);
  const int n = (int)cloudPCL->size();
  std::vector<float> xyz((size_t)3 * n + 3);
  for (int i = 0; i < n; ++i) {
    xyz[3 * (size_t)i] = cloudPCL->points[i].x;
    xyz[3 * (size_t)i + 1] = cloudPCL->points[i].y;
    xyz[3 * (size_t)i + 2] = cloudPCL->points[i].z;
  }
  sfmhip_cloud* dev = nullptr;
  int rc = sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev);
  if (rc != SFMHIP_OK) return rc;
  rc = sfmhip_cloud_ground_plane(dev, labels, label, &o, cam_centres, n_cam, &ground_);
  sfmhip_cloud_destroy(dev);
  return rc;
}

// the options of a levelled call: `opts` (or the defaults) with the frame of the ground plane found over the whole cloud
static int levelled_opts(Dendrometry& d, pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts,
                         const double* cam_centres, int n_cam, const sfmhip_dendro_opts* opts, sfmhip_dendro_opts* out) {
  if (opts)
    *out = *opts;
  else
    sfmhip_dendro_default_opts(out);
  const int rc = d.findGround(cloudPCL, nullptr, 0, cam_centres, n_cam, &ground_opts);
  if (rc != SFMHIP_OK) return rc;
  return sfmhip_dendro_opts_from_ground(&d.ground(), out);
}

int Dendrometry::measure(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label,
                         const sfmhip_ground_opts& ground_opts, const double* cam_centres, int n_cam, const sfmhip_dendro_opts* opts) {
  sfmhip_dendro_opts o;
  const int rc = levelled_opts(*this, cloudPCL, ground_opts, cam_centres, n_cam, opts, &o);
  return rc != SFMHIP_OK ? rc : measure(cloudPCL, labels, label, &o);
}

int Dendrometry::estimateTree(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label,
                              const sfmhip_ground_opts& ground_opts, const double* cam_centres, int n_cam, const sfmhip_dendro_opts* opts) {
  sfmhip_dendro_opts o;
  const int rc = levelled_opts(*this, cloudPCL, ground_opts, cam_centres, n_cam, opts, &o);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_ground_plane: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  return estimateTree(cloudPCL, labels, label, &o);
}

int Dendrometry::findTrees(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_trees_opts& opts) {
  const int n = (int)cloudPCL->size();
  std::vector<float> xyz((size_t)3 * n + 3);
  for (int i = 0; i < n; ++i) {
    xyz[3 * (size_t)i] = cloudPCL->points[i].x;
    xyz[3 * (size_t)i + 1] = cloudPCL->points[i].y;
    xyz[3 * (size_t)i + 2] = cloudPCL->points[i].z;
  }
  sfmhip_cloud* dev = nullptr;
  int rc = sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev);
  if (rc != SFMHIP_OK) return rc;
  treeOf_.assign((size_t)n + 1, -1);
  stems_.assign(4096, sfmhip_tree_stem());
  rc = sfmhip_cloud_trees(dev, labels, label, &opts, treeOf_.data(), (int)stems_.size(), stems_.data(), &trees_);
  treeOf_.resize((size_t)n);
  stems_.resize(rc == SFMHIP_OK ? (size_t)trees_.n_trees : 0);
  sfmhip_cloud_destroy(dev);
  return rc;
}

int Dendrometry::estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts,
                              const double* cam_centres, int n_cam, const sfmhip_trees_opts* trees_opts, const sfmhip_dendro_opts* dendro_opts) {
  sfmhip_dendro_opts d;
  sfmhip_trees_opts t;
  plot_.clear();
  int rc = levelled_opts(*this, cloudPCL, ground_opts, cam_centres, n_cam, dendro_opts, &d);
  if (rc == SFMHIP_OK) {
    if (trees_opts)
      t = *trees_opts;
    else
      sfmhip_trees_default_opts(&t);
    rc = sfmhip_trees_opts_from_ground(&ground_, &t);
  }
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_ground_plane: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  rc = findTrees(cloudPCL, nullptr, 0, t);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_trees: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  std::cout << "************************************************" << std::endl;
  std::cout << "              DENDROMETRY ESTIMATION            " << std::endl;
  std::cout << "************************************************" << std::endl;
  std::cout << "Trees=" << trees_.n_trees << std::endl;
  for (int s = 0; s < trees_.n_trees; ++s) {
    rc = measure(cloudPCL, treeOf_.data(), s, &d);
    if (rc != SFMHIP_OK) {
      std::fprintf(stderr, "[sfm] sfmhip_cloud_dendrometry: %s\n", sfmhip_error_string(rc));
      return rc;
    }
    plot_.push_back(tree_);
    std::cout << "Tree " << s << ": Total Height =" << tree_.total_height << " Altura copa viva=" << tree_.live_crown
              << " Altura base de copa=" << tree_.crown_base_height << " Altura DAP=" << d.dbh_height << " DAP=" << tree_.dbh
              << " Amplitud N-S=" << tree_.spread_ns << " Amplitud E-W=" << tree_.spread_ew << std::endl;
  }
  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
  return rc;
}

int Dendrometry::terrainOn(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_terrain_opts& opts,
                           sfmhip_cloud** keep) {
  const int n = (int)cloudPCL->size();
  std::vector<float> xyz((size_t)3 * n + 3);
  for (int i = 0; i < n; ++i) {
    xyz[3 * (size_t)i] = cloudPCL->points[i].x;
    xyz[3 * (size_t)i + 1] = cloudPCL->points[i].y;
    xyz[3 * (size_t)i + 2] = cloudPCL->points[i].z;
  }
  sfmhip_cloud* dev = nullptr;
  int rc = sfmhip_cloud_create(sfm_hip_context(), n, xyz.data(), &dev);
  if (rc != SFMHIP_OK) return rc;
  isGround_.assign((size_t)n + 1, 0);
  hag_.assign((size_t)n + 1, 0.0f);
  rc = sfmhip_cloud_terrain(dev, labels, label, &opts, isGround_.data(), hag_.data(), &terrain_);
  isGround_.resize((size_t)n);
  hag_.resize((size_t)n);
  if (rc == SFMHIP_OK && keep)
    *keep = dev;
  else
    sfmhip_cloud_destroy(dev);
  return rc;
}

int Dendrometry::findTerrain(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const int* labels, int label, const sfmhip_terrain_opts& opts) {
  return terrainOn(cloudPCL, labels, label, opts, nullptr);
}

int Dendrometry::estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts,
                              const double* cam_centres, int n_cam, const sfmhip_terrain_opts& terrain_opts, const sfmhip_trees_opts* trees_opts,
                              const sfmhip_dendro_opts* dendro_opts) {
  sfmhip_dendro_opts d;
  sfmhip_trees_opts t;
  sfmhip_terrain_opts g = terrain_opts;
  plot_.clear();
  if (dendro_opts)
    d = *dendro_opts;
  else
    sfmhip_dendro_default_opts(&d);
  if (trees_opts)
    t = *trees_opts;
  else
    sfmhip_trees_default_opts(&t);
  int rc = findGround(cloudPCL, nullptr, 0, cam_centres, n_cam, &ground_opts);
  if (rc == SFMHIP_OK) rc = sfmhip_terrain_opts_from_ground(&ground_, &g);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_ground_plane: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  sfmhip_cloud *dev = nullptr, *flat = nullptr;  // the plot, and the plot normalised: born on the device
  rc = terrainOn(cloudPCL, nullptr, 0, g, &dev);
  if (rc == SFMHIP_OK) {
    rc = sfmhip_cloud_terrain_normalize(dev, &flat);
    sfmhip_cloud_destroy(dev);
  }
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_terrain: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  for (int a = 0; a < 3; ++a) {  // on the normalised cloud up is +z, north +y and the ground is at 0
    t.up[a] = d.up[a] = a == 2 ? 1.0 : 0.0;
    t.north[a] = d.north[a] = a == 1 ? 1.0 : 0.0;
  }
  t.ground = d.ground = 0.0;
  const int n = (int)cloudPCL->size();
  treeOf_.assign((size_t)n + 1, -1);
  stems_.assign(4096, sfmhip_tree_stem());
  rc = sfmhip_cloud_trees(flat, nullptr, 0, &t, treeOf_.data(), (int)stems_.size(), stems_.data(), &trees_);
  treeOf_.resize((size_t)n);
  stems_.resize(rc == SFMHIP_OK ? (size_t)trees_.n_trees : 0);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_trees: %s\n", sfmhip_error_string(rc));
    sfmhip_cloud_destroy(flat);
    return rc;
  }
  std::cout << "************************************************" << std::endl;
  std::cout << "              DENDROMETRY ESTIMATION            " << std::endl;
  std::cout << "************************************************" << std::endl;
  std::cout << "Terrain=" << terrain_.De << "x" << terrain_.Dn << " Ground points=" << terrain_.n_ground << std::endl;
  std::cout << "Trees=" << trees_.n_trees << std::endl;
  for (int s = 0; s < trees_.n_trees; ++s) {
    int32_t S = 0;
    profile_.assign(4096, sfmhip_dendro_slice());
    rc = sfmhip_cloud_dendro_profile(flat, treeOf_.data(), s, &d, (int)profile_.size(), profile_.data(), &S, &tree_);
    profile_.resize(rc == SFMHIP_OK ? (size_t)S : 0);
    if (rc != SFMHIP_OK) {
      std::fprintf(stderr, "[sfm] sfmhip_cloud_dendrometry: %s\n", sfmhip_error_string(rc));
      sfmhip_cloud_destroy(flat);
      return rc;
    }
    plot_.push_back(tree_);
    std::cout << "Tree " << s << ": Total Height =" << tree_.total_height << " Altura copa viva=" << tree_.live_crown
              << " Altura base de copa=" << tree_.crown_base_height << " Altura DAP=" << d.dbh_height << " DAP=" << tree_.dbh
              << " Amplitud N-S=" << tree_.spread_ns << " Amplitud E-W=" << tree_.spread_ew << std::endl;
  }
  sfmhip_cloud_destroy(flat);
  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
  return rc;
}

// sfmhip_cloud_crowns on a handle that holds a terrain call: treeOf_, tops_ and crowns_
static int crownsOn(sfmhip_cloud* dev, int n, const sfmhip_crowns_opts& opts, std::vector<int>& treeOf, std::vector<sfmhip_crown_top>& tops,
                    sfmhip_crowns_result& res) {
  treeOf.assign((size_t)n + 1, -1);
  tops.assign((size_t)(opts.max_trees > 0 ? opts.max_trees : 1), sfmhip_crown_top());
  const int rc = sfmhip_cloud_crowns(dev, &opts, treeOf.data(), (int)tops.size(), tops.data(), &res);
  treeOf.resize((size_t)n);
  tops.resize(rc == SFMHIP_OK ? (size_t)(res.n_trees < opts.max_trees ? res.n_trees : opts.max_trees) : 0);
  return rc;
}

int Dendrometry::findCrowns(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_terrain_opts& terrain_opts,
                            const sfmhip_crowns_opts& crown_opts) {
  sfmhip_cloud* dev = nullptr;
  int rc = terrainOn(cloudPCL, nullptr, 0, terrain_opts, &dev);
  if (rc != SFMHIP_OK) return rc;
  rc = crownsOn(dev, (int)cloudPCL->size(), crown_opts, treeOf_, tops_, crowns_);
  sfmhip_cloud_destroy(dev);
  return rc;
}

int Dendrometry::estimatePlot(pcl::PointCloud<pcl::PointXYZRGB>::Ptr& cloudPCL, const sfmhip_ground_opts& ground_opts,
                              const double* cam_centres, int n_cam, const sfmhip_terrain_opts& terrain_opts,
                              const sfmhip_crowns_opts& crown_opts, const sfmhip_dendro_opts* dendro_opts) {
  sfmhip_dendro_opts d;
  sfmhip_terrain_opts g = terrain_opts;
  plot_.clear();
  if (dendro_opts)
    d = *dendro_opts;
  else
    sfmhip_dendro_default_opts(&d);
  int rc = findGround(cloudPCL, nullptr, 0, cam_centres, n_cam, &ground_opts);
  if (rc == SFMHIP_OK) rc = sfmhip_terrain_opts_from_ground(&ground_, &g);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_ground_plane: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  sfmhip_cloud *dev = nullptr, *flat = nullptr;  // the plot, and the plot normalised: born on the device
  rc = terrainOn(cloudPCL, nullptr, 0, g, &dev);
  if (rc != SFMHIP_OK) {
    std::fprintf(stderr, "[sfm] sfmhip_cloud_terrain: %s\n", sfmhip_error_string(rc));
    return rc;
  }
  rc = crownsOn(dev, (int)cloudPCL->size(), crown_opts, treeOf_, tops_, crowns_);
  if (rc != SFMHIP_OK) std::fprintf(stderr, "[sfm] sfmhip_cloud_crowns: %s\n", sfmhip_error_string(rc));
  if (rc == SFMHIP_OK) {
    rc = sfmhip_cloud_terrain_normalize(dev, &flat);
    if (rc != SFMHIP_OK) std::fprintf(stderr, "[sfm] sfmhip_cloud_terrain_normalize: %s\n", sfmhip_error_string(rc));
  }
  sfmhip_cloud_destroy(dev);
  if (rc != SFMHIP_OK) return rc;
  for (int a = 0; a < 3; ++a) {  // on the normalised cloud up is +z, north +y and the ground is at 0
    d.up[a] = a == 2 ? 1.0 : 0.0;
    d.north[a] = a == 1 ? 1.0 : 0.0;
  }
  d.ground = 0.0;
  std::cout << "************************************************" << std::endl;
  std::cout << "              DENDROMETRY ESTIMATION            " << std::endl;
  std::cout << "************************************************" << std::endl;
  std::cout << "Terrain=" << terrain_.De << "x" << terrain_.Dn << " Ground points=" << terrain_.n_ground << std::endl;
  std::cout << "Crowns=" << tops_.size() << " Summits=" << crowns_.n_summits << std::endl;
  for (int s = 0; s < (int)tops_.size(); ++s) {
    int32_t S = 0;
    profile_.assign(4096, sfmhip_dendro_slice());
    rc = sfmhip_cloud_dendro_profile(flat, treeOf_.data(), s, &d, (int)profile_.size(), profile_.data(), &S, &tree_);
    profile_.resize(rc == SFMHIP_OK ? (size_t)S : 0);
    if (rc != SFMHIP_OK) {
      std::fprintf(stderr, "[sfm] sfmhip_cloud_dendrometry: %s\n", sfmhip_error_string(rc));
      sfmhip_cloud_destroy(flat);
      return rc;
    }
    plot_.push_back(tree_);
    std::cout << "Tree " << s << ": Total Height =" << tree_.total_height << " Altura copa viva=" << tree_.live_crown
              << " Altura base de copa=" << tree_.crown_base_height << " Altura DAP=" << d.dbh_height << " DAP=" << tree_.dbh
              << " Amplitud N-S=" << tree_.spread_ns << " Amplitud E-W=" << tree_.spread_ew << " Area de copa=" << tops_[(size_t)s].area
              << std::endl;
  }
  sfmhip_cloud_destroy(flat);
  std::cout << "************************************************" << std::endl;
  std::cout << "************************************************" << std::endl;
  return rc;
}
