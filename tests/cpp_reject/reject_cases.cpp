// wave::ICPMatcher with a correspondence rejector (ICPMatcher::setRejector, include/wave/matching/icp.hpp), built against
// the in-tree libwave_matching.so: the reference's smallDisplacement fixture -- the scan against itself shifted by 0.2 m,
// the transform within 0.1 of the shift in the Frobenius norm (wave_matching/tests/icp_tests.cpp:88-111) -- with each
// rejector, estimateInfo() after it, and a MultiMatcher queue of matchers that take the rejector from the environment.
//
//   usage: reject_cases <repository root> [substring-filter]
//   (the MultiMatcher case wants WAVE_ICP_REJECTOR=trimmed:0.7 in the environment: a pool constructs its matchers itself)
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>
#include <thread>
#include <vector>

#include "wave/matching/icp.hpp"
#include "wave/matching/multi_matcher.hpp"

namespace {

int g_failed = 0;
void expect(bool ok, const char *what, int line) {
    if (ok) return;
    ++g_failed;
    std::printf("reject_cases.cpp:%d: Failure: %s\n", line, what);
}
#define EXPECT(cond) expect((cond), #cond, __LINE__)

std::string g_root = ".";
wave::PCLPointCloudPtr loadScan() {
    auto cloud = boost::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    pcl::io::loadPCDFile(g_root + "/tests/golden/testscan.pcd", *cloud);
    return cloud;
}
wave::PCLPointCloudPtr shifted(const wave::PCLPointCloudPtr &in, const wave::Affine3 &by) {
    auto out = boost::make_shared<pcl::PointCloud<pcl::PointXYZ>>();
    pcl::transformPointCloud(*in, *out, by);
    return out;
}
wave::Affine3 translationX(double dx) {
    wave::Affine3 t = wave::Affine3::Identity();
    t.translation() << dx, 0, 0;
    return t;
}

struct Row {
    const char *name;
    float res;
    double dx;
};
// icp_tests.cpp:49-111: fullResNullMatch, nullDisplacement, smallDisplacement
const Row kRows[] = {{"fullResNullMatch", -1.f, 0.0}, {"nullDisplacement", 0.05f, 0.0}, {"smallDisplacement", 0.05f, 0.2}};

wave::ICPMatcherParams paramsOf(const Row &row) {
    wave::ICPMatcherParams p(g_root + "/tests/golden/config/icp.yaml");
    p.res = row.res;
    // With the default fit_eps = 1e-2 the relative-MSE rule ends a rejecting registration of a scan against its own
    // shifted copy after 4 iterations, 0.19 from the shift: the kept half are the pairs that already lie close, their mean
    // d2 changes by less than 1 % per step (tests/reject_reference.py gives the same 4 iterations and 0.1925).  A
    // rejecting registration wants the tight criterion: 100 iterations, 0.045.
    p.fit_eps = 1e-6;
    return p;
}

typedef wave::ICPMatcher::Rejector Rejector;

void defaultRejector() {
    wave::ICPMatcher m{wave::ICPMatcherParams()};
    EXPECT(m.getRejector() == Rejector::None);
    m.setRejector(Rejector::Trimmed, 0.5);
    EXPECT(m.getRejector() == Rejector::Trimmed);
    wave::ICPMatcher copy(m);  // (MultiMatcher stores copies: the choice travels)
    EXPECT(copy.getRejector() == Rejector::Trimmed);
    wave::ICPMatcher assigned{wave::ICPMatcherParams()};
    assigned = m;
    EXPECT(assigned.getRejector() == Rejector::Trimmed);
    m.setRejector(Rejector::MedianDistance, 1.0);
    EXPECT(m.getRejector() == Rejector::MedianDistance && copy.getRejector() == Rejector::Trimmed);
    m.setRejector(Rejector::None, 0.0);
    EXPECT(m.getRejector() == Rejector::None);
}

void registrations() {
    const auto ref = loadScan();
    const Row &row = kRows[2];  // smallDisplacement
    const wave::Affine3 truth = translationX(row.dx);
    const auto target = shifted(ref, truth);
    struct Choice {
        const char *name;
        Rejector r;
        double value;
    };
    const Choice choices[] = {{"trimmed 0.5", Rejector::Trimmed, 0.5}, {"median 1.0", Rejector::MedianDistance, 1.0}};
    for (const Choice &c : choices) {
        wave::ICPMatcher m(paramsOf(row));
        m.setRejector(c.r, c.value);
        m.setup(ref, target);
        const bool ok = m.match();
        EXPECT(ok);
        const double err = (m.getResult().matrix() - truth.matrix()).norm();
        std::printf("  %s, %s: |T - T_true|_F = %.3e\n", row.name, c.name, err);
        EXPECT(err < 0.1);
        m.estimateInfo();
        EXPECT(m.getInfo()(0, 0) > 0);
    }
    // an invalid ratio is refused: match() returns false, the result stays
    wave::ICPMatcher bad(paramsOf(row));
    bad.setRejector(Rejector::Trimmed, 1.5);
    bad.setup(ref, target);
    EXPECT(!bad.match());
    // not with several devices
    wave::ICPMatcher two(paramsOf(row));
    two.setRejector(Rejector::Trimmed, 0.5);
    two.setDevices({0, 0});
    two.setup(ref, target);
    EXPECT(!two.match());
}

// a queue of pairs through a pool whose matchers take the metric from the environment: the transforms a matcher
// used on each pair alone returns
void multiMatcher() {
    const char *e = std::getenv("WAVE_ICP_REJECTOR");
    EXPECT(e && std::strcmp(e, "trimmed:0.7") == 0);
    const auto ref = loadScan();
    const Row &row = kRows[2];
    wave::ICPMatcherParams p = paramsOf(row);
    std::vector<wave::PCLPointCloudPtr> targets;
    for (int k = 0; k < 4; ++k) targets.push_back(shifted(ref, translationX(0.05 * (k + 1))));
    std::vector<Eigen::Affine3d, Eigen::aligned_allocator<Eigen::Affine3d>> alone;
    for (int k = 0; k < 4; ++k) {
        wave::ICPMatcher m(p);
        EXPECT(m.getRejector() == Rejector::Trimmed);
        m.setup(ref, targets[(size_t) k]);
        EXPECT(m.match());
        alone.push_back(m.getResult());
        EXPECT((m.getResult().matrix() - translationX(0.05 * (k + 1)).matrix()).norm() < 0.1);
    }
    wave::MultiMatcher<wave::ICPMatcher, wave::ICPMatcherParams> pool(2, 10, p);
    for (int k = 0; k < 4; ++k) pool.insert(k, ref, targets[(size_t) k]);
    int id = -1, seen = 0;
    Eigen::Affine3d T;
    wave::Mat6 info;
    while (pool.getResult(&id, &T, &info)) {
        ++seen;
        EXPECT(id >= 0 && id < 4);
        if (id < 0 || id >= 4) continue;
        const double d = (T.matrix() - alone[(size_t) id].matrix()).norm();
        std::printf("  pair %d: |T_pool - T_alone|_F = %.3e\n", id, d);
        EXPECT(d < 1e-12);
        EXPECT(info(0, 0) > 0);
    }
    EXPECT(seen == 4);
}

}  // namespace

int main(int argc, char **argv) {
    if (argc > 1) g_root = argv[1];
    const std::string filter = argc > 2 ? argv[2] : "";
    const std::map<std::string, void (*)()> all = {{"defaultRejector", defaultRejector}, {"registrations", registrations}, {"multiMatcher", multiMatcher}};
    int ran = 0;
    for (const auto &c : all) {
        if (!filter.empty() && c.first.find(filter) == std::string::npos) continue;
        std::printf("[ RUN ] %s\n", c.first.c_str());
        c.second();
        ++ran;
    }
    std::printf("cases run: %d, failed checks: %d\n", ran, g_failed);
    return g_failed == 0 && ran > 0 ? 0 : 1;
}
