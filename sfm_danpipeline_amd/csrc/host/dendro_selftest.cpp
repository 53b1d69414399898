// dendro_selftest.cpp -- the measurement the reference's Dendrometry leaves blank, needs the GPU:
//   dendro_selftest <MAP3D.pcd> <out.bin> [label] [--level[=inlier_tol]]
//   dendro_selftest <MAP3D.pcd> <out.bin> --plot[=inlier_tol]
//   dendro_selftest <MAP3D.pcd> <out.bin> --terrain[=inlier_tol]
//   dendro_selftest <MAP3D.pcd> <out.bin> --crowns[=inlier_tol]
// Without a label: Dendrometry::estimateTree() on every point of the PCD.  With one: the colour segmentation first
// (Segmentation::color_based_growing_segmentation), then estimateTree() on that cluster.  With --level, the ground plane of
// the whole cloud is found first (Dendrometry::findGround, default options or the given tolerance in cloud units) and the
// tree is measured in its frame; without it the output is what it always was.  With --plot, the whole cloud is a plot of
// several trees: Dendrometry::estimatePlot() (ground plane, sfmhip_cloud_trees, one measurement and one printed line per tree).
// out.bin: the sfmhip_dendro_result, i32 slices, then that many sfmhip_dendro_slice rows; with --plot: i32 trees, that many
// sfmhip_tree_stem rows, that many sfmhip_dendro_result, then one i32 tree number per point.  With --terrain the plot stands on
// a terrain: estimatePlot() with default terrain options (ground plane, sfmhip_cloud_terrain in its frame, the trees and the
// measurements on the normalised cloud); out.bin as with --plot, then the sfmhip_terrain_result, one i32 ground flag and one
// float height above ground per point.  With --crowns the trees are found by their crowns, not their stems: estimatePlot() with
// default terrain and crown options (ground plane, sfmhip_cloud_terrain, sfmhip_cloud_crowns on its canopy raster, the
// measurements on the normalised cloud); out.bin: i32 trees, that many sfmhip_crown_top rows, that many sfmhip_dendro_result, one
// i32 tree number per point, then the sfmhip_crowns_result and the sfmhip_terrain_result.
// Exit 3: the cloud is empty or no cluster came out; 4: the library refused the call.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "DendrometryE.h"
#include "Segmentation.h"

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  bool level = false;
  sfmhip_ground_opts gopts;
  sfmhip_ground_default_opts(&gopts);
  if (std::strncmp(argv[argc - 1], "--level", 7) == 0) {
    level = true;
    if (argv[argc - 1][7] == '=') gopts.inlier_tol = std::atof(argv[argc - 1] + 8);
    --argc;
  }
  Dendrometry den;
  int rc;
  if (std::strncmp(argv[argc - 1], "--crowns", 8) == 0) {
    if (argv[argc - 1][8] == '=') gopts.inlier_tol = std::atof(argv[argc - 1] + 9);
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>());
    pcl::io::loadPCDFile(argv[1], *cloud);
    if (cloud->size() <= 0) return 3;
    sfmhip_terrain_opts topts;
    sfmhip_terrain_default_opts(&topts);
    sfmhip_crowns_opts copts;
    sfmhip_crowns_default_opts(&copts);
    if (den.estimatePlot(cloud, gopts, nullptr, 0, topts, copts) != SFMHIP_OK) return 4;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int T = (int)den.tops().size();
    fwrite(&T, 4, 1, o);
    fwrite(den.tops().data(), sizeof(sfmhip_crown_top), (size_t)T, o);
    fwrite(den.plot().data(), sizeof(sfmhip_dendro_result), (size_t)T, o);
    fwrite(den.treeOf().data(), sizeof(int), den.treeOf().size(), o);
    fwrite(&den.crowns(), sizeof(sfmhip_crowns_result), 1, o);
    fwrite(&den.terrain(), sizeof(sfmhip_terrain_result), 1, o);
    fclose(o);
    return 0;
  }
  if (std::strncmp(argv[argc - 1], "--terrain", 9) == 0) {
    if (argv[argc - 1][9] == '=') gopts.inlier_tol = std::atof(argv[argc - 1] + 10);
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>());
    pcl::io::loadPCDFile(argv[1], *cloud);
    if (cloud->size() <= 0) return 3;
    sfmhip_terrain_opts topts;
    sfmhip_terrain_default_opts(&topts);
    if (den.estimatePlot(cloud, gopts, nullptr, 0, topts) != SFMHIP_OK) return 4;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int T = den.trees().n_trees;
    fwrite(&T, 4, 1, o);
    fwrite(den.stems().data(), sizeof(sfmhip_tree_stem), (size_t)T, o);
    fwrite(den.plot().data(), sizeof(sfmhip_dendro_result), (size_t)T, o);
    fwrite(den.treeOf().data(), sizeof(int), den.treeOf().size(), o);
    fwrite(&den.terrain(), sizeof(sfmhip_terrain_result), 1, o);
    fwrite(den.isGround().data(), sizeof(int), den.isGround().size(), o);
    fwrite(den.heightAboveGround().data(), sizeof(float), den.heightAboveGround().size(), o);
    fclose(o);
    return 0;
  }
  if (std::strncmp(argv[argc - 1], "--plot", 6) == 0) {
    if (argv[argc - 1][6] == '=') gopts.inlier_tol = std::atof(argv[argc - 1] + 7);
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>());
    pcl::io::loadPCDFile(argv[1], *cloud);
    if (cloud->size() <= 0) return 3;
    if (den.estimatePlot(cloud, gopts, nullptr, 0) != SFMHIP_OK) return 4;
    FILE* o = fopen(argv[2], "wb");
    if (!o) return 2;
    const int T = den.trees().n_trees;
    fwrite(&T, 4, 1, o);
    fwrite(den.stems().data(), sizeof(sfmhip_tree_stem), (size_t)T, o);
    fwrite(den.plot().data(), sizeof(sfmhip_dendro_result), (size_t)T, o);
    fwrite(den.treeOf().data(), sizeof(int), den.treeOf().size(), o);
    fclose(o);
    return 0;
  }
  if (argc > 3) {
    Segmentation seg;
    seg.setInputFile(argv[1]);
    if (seg.color_based_growing_segmentation() != 0) return 3;
    rc = level ? den.estimateTree(seg.cloud(), seg.labels().data(), std::atoi(argv[3]), gopts, nullptr, 0)
               : den.estimateTree(seg.cloud(), seg.labels().data(), std::atoi(argv[3]));
  } else {
    pcl::PointCloud<pcl::PointXYZRGB>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZRGB>());
    pcl::io::loadPCDFile(argv[1], *cloud);
    if (cloud->size() <= 0) return 3;
    rc = level ? den.estimateTree(cloud, nullptr, 0, gopts, nullptr, 0) : den.estimateTree(cloud, nullptr, 0);
  }
  if (rc != SFMHIP_OK) return 4;
  FILE* o = fopen(argv[2], "wb");
  if (!o) return 2;
  const sfmhip_dendro_result& r = den.tree();
  const int S = (int)den.stemProfile().size();
  fwrite(&r, sizeof r, 1, o);
  fwrite(&S, 4, 1, o);
  fwrite(den.stemProfile().data(), sizeof(sfmhip_dendro_slice), (size_t)S, o);
  fclose(o);
  return 0;
}
