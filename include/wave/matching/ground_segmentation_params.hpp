// Settings of wave::GroundSegmentation (include/wave/matching/ground_segmentation.hpp).
//
// Interface kept from the reference (wave_matching/include/wave/matching/ground_segmentation_params.hpp): the struct
// name, every field with its type and default, and the YAML constructor with its 14 keys.  A file that cannot be
// read logs "Unable to load config" and leaves the defaults of the keys not read (no exception, unlike the matchers'
// constructors).  The fields go to wm_ground_segment unchanged (wm_ground_params, include/wavematch.h).
#ifndef WAVE_GROUNDSEGMENTATIONPARAMS_H
#define WAVE_GROUNDSEGMENTATIONPARAMS_H

#include <string>

namespace wave {

struct GroundSegmentationParams {
    GroundSegmentationParams() {}
    // flat "key: value" YAML file: rmax, num_maxbinpoints, num_seedpoints, num_ang_bins, num_lin_bins,
    // gp_lengthparameter, gp_covariancescale, gp_modelnoise, gp_groundmodelconfidence, gp_grounddataconfidence,
    // gp_groundthreshold, robotheight, seeding_maxrange, seeding_maxheight (libwave_amd/host/ground_segmentation.cpp)
    GroundSegmentationParams(const std::string &config_path);

    // polar grid: points at rmax (m) or farther are ignored; num_bins_a sectors of num_bins_l range bins each
    double rmax = 100;
    int max_bin_points = 200;  // read from the YAML file, not used by the filter (nor by the reference's)
    int num_seed_points = 10;  // lowest eligible cells per sector that start its ground model (< 0: all of them)

    // Gaussian process over (range, height): covariance p_sf * exp(-d^2 / (2 p_l^2)), noise p_sn
    float p_l = 4;
    float p_sf = 1;
    float p_sn = 0.3;
    // a cell joins the ground model when its predicted variance is below p_tmodel and its height lies within
    // p_tdata normalised deviations of the prediction
    float p_tmodel = 5;
    float p_tdata = 5;
    float p_tg = 0.3;  // a point of a model cell within this (m) of the cell's height is ground

    double robot_height = 1.2;  // non-ground points more than this (m) above the ground model are "overhanging"

    // a cell may seed the model only when its range and |height| are below these (m)
    double max_seed_range = 50;
    double max_seed_height = 15;

    int num_bins_a = 72;
    int num_bins_l = 200;
};

}  // namespace wave

#endif  // WAVE_GROUNDSEGMENTATIONPARAMS_H
