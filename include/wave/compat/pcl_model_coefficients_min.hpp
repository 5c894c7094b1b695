// pcl_model_coefficients_min.hpp -- pcl::ModelCoefficients (PCL 1.8 ModelCoefficients.h: the `values` vector; the header
// field is left out) and the constants SACSegmentation<PointT> is configured with (sample_consensus/model_types.h,
// method_types.h: the plane models and SAC_RANSAC, with PCL's values), for builds without PCL.  With PCL installed the
// real headers are used.
#pragma once

#include "wave/compat/pcl_indices_min.hpp"

#if defined(WAVE_MATCHING_USE_SYSTEM_PCL) || __has_include(<pcl/point_cloud.h>)
#include <pcl/ModelCoefficients.h>
#include <pcl/sample_consensus/method_types.h>
#include <pcl/sample_consensus/model_types.h>
#else

#include <vector>

namespace pcl {

struct ModelCoefficients {
    std::vector<float> values;
};

enum SacModel { SACMODEL_PLANE = 0, SACMODEL_PERPENDICULAR_PLANE = 9, SACMODEL_PARALLEL_PLANE = 15 };

const static int SAC_RANSAC = 0;

}  // namespace pcl
#endif
