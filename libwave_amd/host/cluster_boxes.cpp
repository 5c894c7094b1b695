// wave::ClusterBoxes' non-template part and its pcl::PointXYZ instantiation.
#include "wave/matching/cluster_boxes.hpp"

#include <cstring>

#include "shim.hpp"
#include "wave/matching/impl/cluster_boxes.hpp"

namespace wave {

static_assert(sizeof(ClusterBox) == sizeof(wm_cluster_box) && offsetof(ClusterBox, flags) == offsetof(wm_cluster_box, flags) &&
                  offsetof(ClusterBox, aabb_min) == offsetof(wm_cluster_box, aabb_min) &&
                  offsetof(ClusterBox, aabb_max) == offsetof(wm_cluster_box, aabb_max) &&
                  offsetof(ClusterBox, centroid) == offsetof(wm_cluster_box, centroid) &&
                  offsetof(ClusterBox, eigenvalues) == offsetof(wm_cluster_box, eigenvalues) &&
                  offsetof(ClusterBox, axes) == offsetof(wm_cluster_box, axes) &&
                  offsetof(ClusterBox, obb_center) == offsetof(wm_cluster_box, obb_center) &&
                  offsetof(ClusterBox, obb_half) == offsetof(wm_cluster_box, obb_half) &&
                  offsetof(ClusterBox, reserved) == offsetof(wm_cluster_box, reserved) &&
                  (int) ClusterBox::EMPTY == WM_BOX_EMPTY && (int) ClusterBox::NONFINITE == WM_BOX_NONFINITE &&
                  (int) ClusterBox::RANGE == WM_BOX_RANGE,
              "wave::ClusterBox mirrors wm_cluster_box");

namespace detail {

int boxesDefaultDevice() { return shim::defaultDevice(); }

void boxesRelease(wm_ctx *&ctx) { shim::release(ctx); }

bool boxesCompute(wm_ctx *&ctx, int device, const std::vector<const void *> &pts, const std::vector<size_t> &n, size_t stride,
                  const std::vector<const std::vector<pcl::PointIndices> *> &clusters,
                  std::vector<std::vector<ClusterBox>> &out) {
    out.clear();
    const size_t S = pts.size();
    if (clusters.size() != S) {
        LOG_ERROR("ClusterBoxes: %zu clouds but %zu cluster lists", S, clusters.size());
        return false;
    }
    size_t total = 0, n_members = 0, n_clusters = 0;
    for (size_t k = 0; k < S; ++k) {
        if (n[k] == static_cast<size_t>(-1)) {
            LOG_ERROR("ClusterBoxes: cloud %zu is a null pointer", k);
            return false;
        }
        total += n[k];
        n_clusters += clusters[k]->size();
        for (const auto &c : *clusters[k]) n_members += c.indices.size();
    }
    out.resize(S);
    if (n_clusters == 0) return true;
    if (total > 0x7FFFFFF0u || n_members > 0x7FFFFFF0u) {
        LOG_ERROR("ClusterBoxes: more than 0x7FFFFFF0 points or members");
        out.clear();
        return false;
    }
    // one cloud: its records as they are; a queue: the clouds back to back in one array, the indices moved along.
    // An index outside its own cloud is sent as -1, which the device counts as an error whatever the other clouds are.
    std::vector<unsigned char> joined;
    const void *records = S == 1 ? pts[0] : nullptr;
    if (S > 1) {
        joined.resize(total * stride);
        size_t at = 0;
        for (size_t k = 0; k < S; ++k) {
            if (n[k]) std::memcpy(joined.data() + at * stride, pts[k], n[k] * stride);
            at += n[k];
        }
        records = total ? joined.data() : nullptr;
    }
    std::vector<int32_t> indices;
    std::vector<uint32_t> offsets;
    indices.reserve(n_members);
    offsets.reserve(n_clusters + 1);
    offsets.push_back(0);
    size_t base = 0;
    for (size_t k = 0; k < S; ++k) {
        for (const auto &c : *clusters[k]) {
            for (const int i : c.indices)
                indices.push_back(i >= 0 && (size_t) i < n[k] ? (int32_t) (base + (size_t) i) : (int32_t) -1);
            offsets.push_back((uint32_t) indices.size());
        }
        base += n[k];
    }
    if (!shim::acquire(ctx, device)) {
        out.clear();
        return false;
    }
    std::vector<wm_cluster_box> boxes(n_clusters);
    static const int32_t none = 0;  // (a non-null pointer for an empty member list: NULL would mean "record e")
    const int rc = wm_cluster_boxes(ctx, records, total, stride, WM_MEM_HOST, indices.empty() ? &none : indices.data(),
                                    indices.size(), offsets.data(), n_clusters, WM_MEM_HOST, boxes.data(), WM_MEM_HOST, nullptr);
    if (rc != WM_OK) {
        LOG_ERROR("wm_cluster_boxes failed: %s [%s]", wm_strerror(rc), wm_last_error(ctx));
        out.clear();
        return false;
    }
    size_t at = 0;
    for (size_t k = 0; k < S; ++k) {
        out[k].resize(clusters[k]->size());
        if (!out[k].empty()) std::memcpy(static_cast<void *>(out[k].data()), &boxes[at], out[k].size() * sizeof(ClusterBox));
        at += out[k].size();
    }
    return true;
}

}  // namespace detail

template class ClusterBoxes<pcl::PointXYZ>;

}  // namespace wave
