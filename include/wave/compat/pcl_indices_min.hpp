// pcl_indices_min.hpp -- pcl::PointIndices (PCL 1.8 PointIndices.h: the `indices` vector; the header field is left
// out), which EuclideanClusterExtraction<PointT>::extract returns its clusters in, for builds without PCL.  With PCL
// installed the real header is used.
#pragma once

#include "wave/compat/pcl_min.hpp"

#if defined(WAVE_MATCHING_USE_SYSTEM_PCL) || __has_include(<pcl/point_cloud.h>)
#include <pcl/PointIndices.h>
#else

#include <vector>

namespace pcl {

struct PointIndices {
    std::vector<int> indices;
};

}  // namespace pcl
#endif
