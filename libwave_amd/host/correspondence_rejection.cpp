// wave::CorrespondenceRejectorSampleConsensus's non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/correspondence_rejection.hpp"

#include <cmath>

#include "shim.hpp"
#include "wave/matching/impl/correspondence_rejection.hpp"

namespace wave {

CorrespondenceRejectionParams::CorrespondenceRejectionParams(const std::string &config_path) {
    try {
        shim::loadYaml(config_path, {{"inlier_threshold", &inlier_threshold},
                                     {"max_iterations", &max_iterations},
                                     {"probability", &probability},
                                     {"refine_model", &refine_model},
                                     {"min_sample_distance", &min_sample_distance}});
    } catch (const std::runtime_error &) {
        LOG_ERROR("Unable to load config");  // (as FPFHParams: log and carry on with what is there)
    }
}

namespace detail {

int corrDefaultDevice() { return shim::defaultDevice(); }

void corrRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool corrRansac(wm_ctx *&ctx, int device, const void *src, size_t n_src, const void *tgt, size_t n_tgt, size_t stride,
                const CorrespondenceRejectionParams &params, const std::vector<pcl::Correspondence> &in,
                std::vector<pcl::Correspondence> &remaining, double T[16]) {
    remaining.clear();
    if (!src || !tgt || n_src == 0 || n_tgt == 0) {
        LOG_ERROR("getRemainingCorrespondences: the source and the target cloud must be set and not empty");
        return false;
    }
    if (!std::isfinite(params.inlier_threshold) || !(params.inlier_threshold > 0) || params.max_iterations < 1 ||
        !(params.probability > 0 && params.probability < 1) || !std::isfinite(params.min_sample_distance)) {
        LOG_ERROR("getRemainingCorrespondences: inlier_threshold = %g must be > 0, max_iterations = %d >= 1, probability = %g in "
                  "(0, 1), min_sample_distance = %g finite",
                  params.inlier_threshold, params.max_iterations, params.probability, params.min_sample_distance);
        return false;
    }
    if (in.size() > WM_FEATURE_MAX_ROWS) {
        LOG_ERROR("getRemainingCorrespondences: %zu correspondences, at most %u", in.size(), WM_FEATURE_MAX_ROWS);
        return false;
    }
    if (in.size() < 3) return false;  // (no sample: no model, no device)
    std::vector<int32_t> query(in.size()), match(in.size()), kept(in.size());
    for (size_t e = 0; e < in.size(); ++e) {
        query[e] = in[e].index_query;
        match[e] = in[e].index_match;
    }
    if (!shim::acquire(ctx, device)) return false;
    wm_corr_ransac_params p;
    wm_corr_ransac_default_params(&p);
    p.inlier_threshold = params.inlier_threshold;
    p.max_iterations = params.max_iterations;
    p.probability = params.probability;
    p.refine_model = params.refine_model;
    p.min_sample_distance = params.min_sample_distance;
    p.seed = params.seed;
    size_t n_out = 0;
    const int rc = wm_corr_ransac(ctx, src, n_src, tgt, n_tgt, stride, query.data(), match.data(), in.size(), WM_MEM_HOST, &p, T,
                                  kept.data(), kept.size(), WM_MEM_HOST, &n_out, nullptr, nullptr);
    if (rc == WM_NOT_CONVERGED) return false;
    if (rc != WM_OK) {
        LOG_ERROR("wm_corr_ransac failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        return false;
    }
    remaining.reserve(n_out);
    for (size_t k = 0; k < n_out; ++k) remaining.push_back(in[(size_t) kept[k]]);
    return true;
}

}  // namespace detail

template class CorrespondenceRejectorSampleConsensus<pcl::PointXYZ>;

}  // namespace wave
