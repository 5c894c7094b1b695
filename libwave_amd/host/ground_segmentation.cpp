// wave::GroundSegmentation's non-template part and its pcl::PointXYZ instantiation
// (wave_matching/src/ground_segmentation.cpp:8 precompiles PCL_XYZ_POINT_TYPES).
#include "wave/matching/ground_segmentation.hpp"

#include "shim.hpp"
#include "wave/matching/impl/ground_segmentation.hpp"

namespace wave {

GroundSegmentationParams::GroundSegmentationParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"rmax", &rmax},
                                     {"num_maxbinpoints", &max_bin_points},
                                     {"num_seedpoints", &num_seed_points},
                                     {"num_ang_bins", &num_bins_a},
                                     {"num_lin_bins", &num_bins_l},
                                     {"gp_lengthparameter", &p_l},
                                     {"gp_covariancescale", &p_sf},
                                     {"gp_modelnoise", &p_sn},
                                     {"gp_groundmodelconfidence", &p_tmodel},
                                     {"gp_grounddataconfidence", &p_tdata},
                                     {"gp_groundthreshold", &p_tg},
                                     {"robotheight", &robot_height},
                                     {"seeding_maxrange", &max_seed_range},
                                     {"seeding_maxheight", &max_seed_height}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (the reference logs and carries on with what it has)
    }
}

namespace detail {

int groundDefaultDevice() { return shim::defaultDevice(); }

void groundRelease(wm_ctx *&ctx) { shim::release(ctx); }

static wm_ground_params groundParams(const GroundSegmentationParams &params) {
    wm_ground_params p;
    p.rmax = params.rmax;
    p.max_bin_points = params.max_bin_points;
    p.num_seed_points = params.num_seed_points;
    p.p_l = params.p_l;
    p.p_sf = params.p_sf;
    p.p_sn = params.p_sn;
    p.p_tmodel = params.p_tmodel;
    p.p_tdata = params.p_tdata;
    p.p_tg = params.p_tg;
    p.robot_height = params.robot_height;
    p.max_seed_range = params.max_seed_range;
    p.max_seed_height = params.max_seed_height;
    p.num_bins_a = params.num_bins_a;
    p.num_bins_l = params.num_bins_l;
    return p;
}

bool groundSegmentIndices(wm_ctx *&ctx, int device, const void *pts, size_t n, size_t stride,
                          const GroundSegmentationParams &params, bool keep_ground, bool keep_obs, bool keep_drv,
                          std::vector<int> &out) {
    out.clear();
    const wm_ground_params p = groundParams(params);
    if (!shim::acquire(ctx, device)) return false;
    const int keep = (keep_ground ? WM_KEEP_GROUND : 0) | (keep_obs ? WM_KEEP_OBSTACLE : 0) |
                     (keep_drv ? WM_KEEP_OVERHANGING : 0);
    out.resize(n);
    size_t m = 0;
    const int rc = wm_ground_segment(ctx, pts, n, stride, WM_MEM_HOST, &p, keep,
                                     n ? reinterpret_cast<int32_t *>(out.data()) : nullptr, n, WM_MEM_HOST, &m,
                                     nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_ground_segment failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        out.clear();
        return false;
    }
    out.resize(m);
    return true;
}

void groundLogNullScan(size_t k) { LOG_ERROR("GroundSegmentation::filterBatch: input %zu is null", k); }

bool groundSegmentIndicesBatch(wm_ctx *&ctx, int device, const void *const *pts, const size_t *n, size_t count,
                               size_t stride, const GroundSegmentationParams &params, bool keep_ground, bool keep_obs,
                               bool keep_drv, std::vector<std::vector<int>> &out) {
    out.assign(count, std::vector<int>());
    if (count == 0) return true;
    const wm_ground_params p = groundParams(params);
    if (count > 0x7FFFFFFFu) {
        LOG_ERROR("wm_ground_segment_batch: too many scans");
        return false;
    }
    if (!shim::acquire(ctx, device)) return false;
    const int keep = (keep_ground ? WM_KEEP_GROUND : 0) | (keep_obs ? WM_KEEP_OBSTACLE : 0) |
                     (keep_drv ? WM_KEEP_OVERHANGING : 0);
    std::vector<wm_ground_scan> scans(count);
    size_t total = 0;
    for (size_t k = 0; k < count; ++k) {
        scans[k].pts = pts[k];
        scans[k].n = n[k];
        total += n[k];
    }
    std::vector<int32_t> idx(total ? total : 1);
    std::vector<size_t> offsets(count + 1, 0);
    const int rc = wm_ground_segment_batch(ctx, scans.data(), static_cast<int>(count), stride, WM_MEM_HOST, &p, keep,
                                           idx.data(), total, nullptr, 0, WM_MEM_HOST, offsets.data(), nullptr,
                                           nullptr, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_ground_segment_batch failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    for (size_t k = 0; k < count; ++k) out[k].assign(idx.begin() + offsets[k], idx.begin() + offsets[k + 1]);
    return true;
}

}  // namespace detail

template class GroundSegmentation<pcl::PointXYZ>;  // (the reference precompiles every PCL XYZ type)

}  // namespace wave
