// Host unit test (no device): trajectoryPositionRMSE (eqvio_amd/host/DatasetReplay.hpp) - the position RMSE of an estimated trajectory against ground truth
// after aligning the first poses.
#include "DatasetReplay.hpp"
#include <cmath>
#include <cstdio>
#include <cstdlib>

using namespace eqvio_amd;
using eqf::Pose;
using eqf::Qt;
using eqf::V3;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            std::fprintf(stderr, "FAILED %s (line %d)\n", #cond, __LINE__); \
            std::exit(1);                                                   \
        }                                                                   \
    } while (0)

static Pose curve(double t) { // a pose that turns and moves a few metres
    const V3 w{0.3 * t, -0.2 * t, 0.5 * t};
    return Pose{eqf::so3_exp(w), V3{2.0 * std::sin(0.7 * t), 1.5 * std::cos(0.4 * t) - 1.5, 0.8 * t}};
}

int main() {
    const int F = 40;
    std::vector<StampedPose> gt(F);
    double extent = 0.0;
    for (int j = 0; j < F; ++j) {
        gt[j].t = 10.0 + 0.05 * j;
        gt[j].pose = curve(0.05 * j);
        extent = std::fmax(extent, eqf::norm(gt[j].pose.x - gt[0].pose.x));
    }
    CHECK(extent > 1.0);
    // an estimate that is a rigid transform of the ground truth: e_j = T^-1 g_j, so A = g_0 e_0^-1 = T
    const Pose T{eqf::so3_exp(V3{0.4, -1.1, 0.7}), V3{3.0, -2.0, 0.5}};
    std::vector<StampedPose> est(F);
    for (int j = 0; j < F; ++j) {
        est[j].t = gt[j].t;
        est[j].pose = eqf::pose_mul(eqf::pose_inv(T), gt[j].pose);
    }
    TrajectoryScore s = trajectoryPositionRMSE(est, gt);
    std::printf("rigid %.3e extent %.3f\n", s.rmse, extent);
    CHECK(s.frames == F && s.rmse <= 1e-12 * extent);
    // a constant offset d (in the aligned frame) from the second frame on: d sqrt((F - 1) / F)
    const V3 off{0.03, -0.04, 0.12};
    const double d = eqf::norm(off);
    std::vector<StampedPose> shifted = est;
    for (int j = 1; j < F; ++j)
        shifted[j].pose.x = shifted[j].pose.x + eqf::q_rot(eqf::q_inv(T.R), off);
    s = trajectoryPositionRMSE(shifted, gt);
    std::printf("offset %.17g expected %.17g\n", s.rmse, d * std::sqrt((F - 1.0) / F));
    CHECK(s.frames == F && std::fabs(s.rmse - d * std::sqrt((F - 1.0) / F)) <= 1e-12 * extent);
    // rows with stamp -1 (a filter that has not initialised) are skipped, wherever they stand: the first kept frame aligns
    std::vector<StampedPose> led;
    StampedPose none;
    none.t = -1.0;
    none.pose = Pose{eqf::q_identity(), V3{100.0, 100.0, 100.0}};
    led.push_back(none);
    led.push_back(none);
    led.insert(led.end(), est.begin(), est.end());
    led.insert(led.begin() + 10, none);
    s = trajectoryPositionRMSE(led, gt);
    CHECK(s.frames == F && s.rmse <= 1e-12 * extent);
    // the nearest ground-truth pose; on a tie the earlier one
    std::vector<StampedPose> g3(3);
    for (int j = 0; j < 3; ++j) {
        g3[j].t = 1.0 + j; // 1, 2, 3: exact in binary, and so are the midpoints
        g3[j].pose = Pose{eqf::q_identity(), V3{(double)(j * j), 0.0, 0.0}}; // x = 0, 1, 4
    }
    std::vector<StampedPose> e2(2);
    e2[0].t = 1.0, e2[0].pose = Pose{eqf::q_identity(), V3{0.0, 0.0, 0.0}};
    e2[1].t = 2.5, e2[1].pose = Pose{eqf::q_identity(), V3{1.0, 0.0, 0.0}}; // tie between stamps 2 (x = 1) and 3 (x = 4): the earlier
    s = trajectoryPositionRMSE(e2, g3);
    CHECK(s.frames == 2 && s.rmse == 0.0);
    e2[1].t = 2.75; // nearer to 3: error 3 in one of two frames
    s = trajectoryPositionRMSE(e2, g3);
    CHECK(std::fabs(s.rmse - 3.0 / std::sqrt(2.0)) <= 1e-15);
    e2[1].t = 1.5, e2[1].pose.x = V3{0.0, 0.0, 0.0}; // tie between stamps 1 and 2: the earlier (x = 0)
    s = trajectoryPositionRMSE(e2, g3);
    CHECK(s.rmse == 0.0);
    e2[1].t = 99.0, e2[1].pose.x = V3{4.0, 0.0, 0.0}; // beyond the last stamp: the last pose
    CHECK(trajectoryPositionRMSE(e2, g3).rmse == 0.0);
    // the same rule on ground truth that is not in stamp order (a scan in file order)
    std::vector<StampedPose> g3r{g3[2], g3[0], g3[1]};
    e2[1].t = 2.5, e2[1].pose.x = V3{4.0, 0.0, 0.0}; // tie between 3 (first in the file) and 2: the earlier in the file
    CHECK(trajectoryPositionRMSE(e2, g3r).rmse == 0.0);
    // nothing to score
    s = trajectoryPositionRMSE({}, gt);
    CHECK(std::isnan(s.rmse) && s.frames == 0);
    s = trajectoryPositionRMSE({none, none}, gt);
    CHECK(std::isnan(s.rmse) && s.frames == 0);
    s = trajectoryPositionRMSE(est, {});
    CHECK(std::isnan(s.rmse) && s.frames == 0);
    std::puts("ok");
    return 0;
}
