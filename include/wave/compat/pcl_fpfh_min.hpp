// pcl_fpfh_min.hpp -- pcl::FPFHSignature33 (PCL 1.8 point_types.hpp: `float histogram[33]`) and pcl::Correspondence
// (PCL 1.8 correspondence.h: index_query, index_match, distance), which wave::FPFHEstimation<PointT>::compute and
// wave::matchFeatures return their results in, for builds without PCL.  With PCL installed the real headers are used.
#pragma once

#include "wave/compat/pcl_min.hpp"

#if defined(WAVE_MATCHING_USE_SYSTEM_PCL) || __has_include(<pcl/point_cloud.h>)
#include <pcl/correspondence.h>
#include <pcl/point_types.h>
#else

namespace pcl {

struct FPFHSignature33 {
    float histogram[33];
    static int descriptorSize() { return 33; }
};

struct Correspondence {
    int index_query = 0;   // a row of the first set
    int index_match = -1;  // its match in the second
    float distance = 0.f;  // the SQUARED distance between the two descriptors, as PCL's estimators store it
    Correspondence() {}
    Correspondence(int query, int match, float d) : index_query(query), index_match(match), distance(d) {}
};

}  // namespace pcl
#endif
