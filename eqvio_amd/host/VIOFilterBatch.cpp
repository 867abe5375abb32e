// VIOFilterBatch (VIOFilterBatch.hpp) and its C-ABI (include/eqvio_batch.h).
#include "VIOFilterBatch.hpp"
#include "eqvio_batch.h"
#include "PreparedFrames.hpp"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <array>
#include <map>
#include <memory>
#include <sys/stat.h>
#include <stdexcept>
#include <string>

namespace eqvio_amd {

std::vector<double> imuDts(const std::vector<IMUVelocity>& buffer, double currentTime, double newTime) { // VIOFilter.cpp:137-145, VIO_eqf.cpp:142-147
    std::vector<double> dts(buffer.size());
    for (size_t i = 0; i < buffer.size(); ++i) {
        const double t0 = std::max(buffer.at(i).stamp, currentTime);
        const double t1 = i + 1 < buffer.size() ? std::min(buffer.at(i + 1).stamp, newTime) : newTime;
        dts[i] = std::max(t1 - t0, 0.0);
    }
    return dts;
}
ImuSelection selectImu(const std::vector<IMUVelocity>& buffer, double currentTime, double newTime) { // VIOFilter.cpp:134-156
    ImuSelection s;
    s.dts = imuDts(buffer, currentTime, newTime);
    IMUVelocity acc = IMUVelocity::Zero();
    for (size_t i = 0; i < buffer.size(); ++i) {
        s.total += s.dts[i];
        acc = acc + buffer.at(i) * s.dts[i];
    }
    s.mean = acc * (1.0 / s.total);
    return s;
}
void trimImuBuffer(std::vector<IMUVelocity>& buffer, double currentTime) { // VIOFilter.cpp:182-189
    auto it = std::find_if(buffer.begin(), buffer.end(), [currentTime](const IMUVelocity& v) { return v.stamp >= currentTime; });
    if (it != buffer.begin()) {
        --it;
        buffer.erase(buffer.begin(), it);
    }
}

void writeConsistencyRecord(VIOWriter& writer, double stamp, const eqf_batch_consistency_record& r, int n_true, const int* true_ids) {
    writer.writeNEESRow(stamp, r.nees, 21 + 3 * r.N, r.block[EQF_BLOCK_POSE], r.block[EQF_BLOCK_ATTITUDE]);
    const auto rows = [&](VIOWriter::ConsistencyFile which, int s0) {
        double eps[6], sigma2[6];
        for (int k = 0; k < 6; ++k)
            eps[k] = r.eps[s0 + k], sigma2[k] = r.sigma_diag[s0 + k];
        writer.writeConsistencyRow(which, stamp, eps, sigma2);
    };
    rows(VIOWriter::PoseConsistency, 6);
    rows(VIOWriter::CameraConsistency, 15);
    rows(VIOWriter::BiasConsistency, 0);
    std::map<int, double> held;
    for (int i = 0; i < r.N; ++i)
        held.emplace(r.ids[i], r.lm_err[i]);
    std::vector<double> errors(n_true);
    for (int j = 0; j < n_true; ++j) {
        const auto it = held.find(true_ids[j]);
        errors[j] = it == held.end() ? std::nan("") : it->second;
    }
    writer.writeLandmarkErrorRow(stamp, errors);
}

void writeEstimateRecord(VIOWriter& writer, double stamp, const eqf_batch_estimate_record& r) {
    writer.writeSensorRows(stamp, r.sensor);
    writer.writePointsRow(stamp, r.N, r.ids, r.p_world);
}
std::unique_ptr<VIOWriter> makeRunWriter(const std::string& output_dir, int k) {
    const std::string dir = output_dir + "/run_" + std::to_string(k);
    auto writer = std::make_unique<VIOWriter>(dir);
    struct stat st;
    if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
        throw std::runtime_error("cannot create the output directory " + dir);
    for (const char* name : {"IMUState.csv", "camera.csv", "bias.csv", "points.csv"})
        std::remove((dir + "/" + name).c_str());
    return writer;
}

namespace {
// constructInitialStateCovarianceDiag (VIOFilterSettings.h:208-229)
std::vector<double> initialCovariance(const eqvio_settings& s, int N) {
    std::vector<double> d(21 + 3 * (size_t)N, s.initialPointVariance);
    const double v[7] = {s.initialBiasOmegaVariance, s.initialBiasAccelVariance, s.initialAttitudeVariance, s.initialPositionVariance,
                         s.initialVelocityVariance,  s.initialCameraAttitudeVariance, s.initialCameraPositionVariance};
    for (int b = 0; b < 7; ++b)
        for (int k = 0; k < 3; ++k)
            d[3 * b + k] = v[b];
    if (s.initialPointDepthVariance > 0)
        for (int i = 0; i < N; ++i)
            d[21 + 3 * i + 2] = s.initialPointDepthVariance;
    return d;
}
std::vector<double> diagonal(const std::vector<double>& d) {
    const size_t n = d.size();
    std::vector<double> m(n * n, 0.0);
    for (size_t i = 0; i < n; ++i)
        m[i * n + i] = d[i];
    return m;
}
const double kIdentityGroup[23] = {0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0};
struct BatchFailure : std::runtime_error {
    int code;
    BatchFailure(const std::string& m, int c) : std::runtime_error(m), code(c) {}
};
void check(int rc, const char* what) {
    if (rc != 0)
        throw BatchFailure(std::string(what) + ": " + eqf_error_string(rc), rc);
}
} // namespace

VIOFilterBatch::VIOFilterBatch(eqf_batch* b) : batch(b) {
    const int slots = eqf_batch_slots(b);
    slotv.resize(slots);
    riccati_.assign(slots, EQVIO_BATCH_RICCATI_FAST);
    stateMatrix_.assign(slots, EQVIO_BATCH_STATE_MATRIX_CONTINUOUS);
    for (int k = 0; k < slots; ++k) {
        try {
            resetSlot(k);
        } catch (const BatchFailure&) {
            eqf_batch_destroy(batch);
            batch = nullptr;
            throw;
        }
    }
}
VIOFilterBatch::~VIOFilterBatch() { eqf_batch_destroy(batch); }

eqvio_settings VIOFilterBatch::slotSettings(int k) const {
    eqvio_settings s;
    check(eqf_batch_get_slot_settings(batch, k, &s), "eqf_batch_get_slot_settings");
    return s;
}
int VIOFilterBatch::setRiccatiMode(int k, int mode) {
    if ((mode != EQVIO_BATCH_RICCATI_FAST && mode != EQVIO_BATCH_RICCATI_ACCURATE) || k >= (int)slotv.size())
        return EQF_E_BAD_ARG;
    if (k < 0)
        riccati_.assign(slotv.size(), mode);
    else
        riccati_[k] = mode;
    return 0;
}
int VIOFilterBatch::riccatiMode(int k) const { return k >= 0 && k < (int)slotv.size() ? riccati_[k] : EQF_E_BAD_ARG; }
int VIOFilterBatch::setStateMatrix(int k, int kind) {
    if ((kind != EQVIO_BATCH_STATE_MATRIX_CONTINUOUS && kind != EQVIO_BATCH_STATE_MATRIX_DISCRETE) || k >= (int)slotv.size())
        return EQF_E_BAD_ARG;
    if (k < 0)
        stateMatrix_.assign(slotv.size(), kind);
    else
        stateMatrix_[k] = kind;
    return 0;
}
int VIOFilterBatch::callOf(int k) const { // integrateUpToTime's choice (src/VIOFilter.cpp:160-178): the state matrix matters to an accurate slot only
    return riccati_[k] != EQVIO_BATCH_RICCATI_ACCURATE ? 0 : stateMatrix_[k] == EQVIO_BATCH_STATE_MATRIX_DISCRETE ? 2 : 1;
}
int VIOFilterBatch::stateMatrix(int k) const { return k >= 0 && k < (int)slotv.size() ? stateMatrix_[k] : EQF_E_BAD_ARG; }
int VIOFilterBatch::groupOf(int k) const { return 2 * callOf(k) + (eqf_batch_get_slot_chart(batch, k) == EQVIO_COORD_NORMAL ? 1 : 0); }
int VIOFilterBatch::setChart(int k, int chart) {
    if (k >= (int)slotv.size() || (chart != EQVIO_COORD_EUCLIDEAN && chart != EQVIO_COORD_INVDEPTH && chart != EQVIO_COORD_NORMAL))
        return EQF_E_BAD_ARG;
    if (k >= 0)
        return eqf_batch_set_slot_chart(batch, k, chart);
    for (int j = 0; j < (int)slotv.size(); ++j) // every slot, or none: the one refusal left is a slot with landmarks under another chart
        if (eqf_batch_get_slot_chart(batch, j) != chart && eqf_batch_num_landmarks(batch, j) > 0)
            return EQF_E_BAD_ARG;
    for (int j = 0; j < (int)slotv.size(); ++j)
        if (const int rc = eqf_batch_set_slot_chart(batch, j, chart))
            return rc;
    return 0;
}
int VIOFilterBatch::chart(int k) const { return eqf_batch_get_slot_chart(batch, k); }
int VIOFilterBatch::convertChart(int count, const int* slots, const int* charts, int* status) { return eqf_batch_convert_chart(batch, count, slots, charts, status); }
VIOFilterBatch::InnovationTotals VIOFilterBatch::innovationTotals(int k) const {
    InnovationTotals t;
    check(eqf_batch_innovation_totals(batch, k, &t.updates, &t.dof, &t.nis, &t.logdet), "eqf_batch_innovation_totals");
    return t;
}
// VIOFilter(const Settings&) (VIOFilter.cpp:31-41) with the slot's settings: xi0 with the camera offset, X = identity, Sigma = the initial sensor covariance
void VIOFilterBatch::resetSlot(int k) {
    const eqvio_settings s = slotSettings(k);
    double xi0[23];
    std::memcpy(xi0, kIdentityGroup, sizeof(xi0));
    std::memcpy(xi0 + 16, s.cameraOffset, sizeof(double) * 7);
    const std::vector<double> S = diagonal(initialCovariance(s, 0));
    const int rc = eqf_batch_set_state(batch, k, xi0, kIdentityGroup, nullptr, nullptr, nullptr, 0);
    check(rc ? rc : eqf_batch_set_sigma(batch, k, S.data(), 21), "eqf_batch_set_state / eqf_batch_set_sigma");
}
int VIOFilterBatch::setSlotSettings(int k, const eqvio_settings& s) {
    if (const int rc = eqf_batch_check_settings(&s)) // the refusals in the order eqf_batch.h documents: the settings on their own first,
        return rc;
    eqvio_settings old;
    if (const int rc = eqf_batch_get_slot_settings(batch, k, &old)) // ... then the slot index,
        return rc;
    if (const int rc = eqf_batch_set_slot_settings(batch, k, &s)) // ... then the chart against the slot's landmarks
        return rc;
    // what resetSlot reads of the settings: only a change of these asks for a new initial state
    const bool initialValuesChanged = std::memcmp(old.cameraOffset, s.cameraOffset, sizeof(old.cameraOffset)) != 0 || initialCovariance(old, 0) != initialCovariance(s, 0);
    if (!slotv.at(k).initialised && initialValuesChanged && eqf_batch_num_landmarks(batch, k) == 0) {
        try {
            resetSlot(k);
        } catch (const BatchFailure&) {
            if (const int rc = eqf_batch_set_slot_settings(batch, k, &old)) // N = 0: no chart refusal, so the slot has its former settings again
                throw BatchFailure(std::string("the slot's reset failed, and so did putting its former settings back: ") + eqf_error_string(rc), rc);
            throw;
        }
    }
    return 0;
}

// eqf_batch_copy_slots, then the host half of every entry that was done, from the sources as they were before the call
void VIOFilterBatch::copySlots(int count, const int* src, const int* dst, int* status) {
    check(eqf_batch_copy_slots(batch, count, src, dst, status), "eqf_batch_copy_slots");
    std::vector<Slot> held(count);
    for (int e = 0; e < count; ++e)
        if (status[e] == 0 && src[e] != dst[e])
            held[e] = slotv.at(src[e]);
    for (int e = 0; e < count; ++e)
        if (status[e] == 0 && src[e] != dst[e])
            slotv.at(dst[e]) = std::move(held[e]);
}

int VIOFilterBatch::loadFilter(VIOFilter& src, int count, const int* slots, int* status) {
    src.eqfState().settleInvalid(); // what every view of the filter's state does first
    if (const int rc = eqf_batch_load_ctx(batch, src.eqfState().ctx, count, slots, status))
        return rc;
    for (int e = 0; e < count; ++e)
        if (status[e] == 0) {
            Slot& sl = slotv.at(slots[e]);
            sl.velocityBuffer = src.imuBuffer();
            sl.currentTime = src.getTime();
            sl.initialised = src.isInitialised();
        }
    return 0;
}
int VIOFilterBatch::storeFilter(int k, VIOFilter& dst) {
    dst.eqfState().settleInvalid(); // a deferred removal belongs to the state that is about to be replaced: done, not carried over
    if (const int rc = eqf_batch_store_ctx(batch, k, dst.eqfState().ctx))
        return rc;
    const Slot& sl = slotv.at(k);
    dst.adoptHostState(sl.velocityBuffer, sl.currentTime, sl.initialised);
    return 0;
}
void VIOFilterBatch::startFromState(int k, const double* sensor, const int* ids, const double* p, int N, double time) { // VIOFilter.cpp:43-56
    Slot& sl = slotv.at(k);
    std::vector<double> Q(5 * (size_t)N);
    for (int i = 0; i < N; ++i) {
        const double q[5] = {1, 0, 0, 0, 1};
        std::memcpy(Q.data() + 5 * i, q, sizeof(q));
    }
    check(eqf_batch_set_state(batch, k, sensor, kIdentityGroup, ids, p, Q.data(), N), "eqf_batch_set_state");
    const std::vector<double> S = diagonal(initialCovariance(slotSettings(k), N));
    check(eqf_batch_set_sigma(batch, k, S.data(), 21 + 3 * N), "eqf_batch_set_sigma");
    sl.velocityBuffer.clear();
    sl.currentTime = time;
    sl.initialised = true;
}
void VIOFilterBatch::processIMUData(int k, const IMUVelocity& imu) { // VIOFilter.cpp:58-63
    Slot& sl = slotv.at(k);
    if (!sl.initialised)
        initialiseFromIMUData(k, imu);
    sl.velocityBuffer.emplace_back(imu);
}
void VIOFilterBatch::initialiseFromIMUData(int k, const IMUVelocity& imu) { // VIOFilter.cpp:65-78
    const int N = eqf_batch_num_landmarks(batch, k);
    std::vector<double> xi0(23), X(23), q0(3 * (size_t)N), Q(5 * (size_t)N);
    std::vector<int> ids(N);
    check(eqf_batch_get_state(batch, k, xi0.data(), X.data(), ids.data(), q0.data(), Q.data(), N) < 0 ? -1 : 0, "eqf_batch_get_state");
    for (int i = 0; i < 6; ++i)
        xi0[i] = 0.0;
    const Qt R = so3_from_vectors(normalized(imu.acc), V3{0, 0, 1});
    const double pose[7] = {R.w, R.x, R.y, R.z, 0, 0, 0};
    std::memcpy(xi0.data() + 6, pose, sizeof(pose));
    xi0[13] = xi0[14] = xi0[15] = 0.0;
    check(eqf_batch_set_state(batch, k, xi0.data(), X.data(), ids.data(), q0.data(), Q.data(), N), "eqf_batch_set_state");
    slotv.at(k).initialised = true;
    slotv.at(k).currentTime = imu.stamp;
}

// processVisionData's early returns (VIOFilter.cpp:135-136, 198-199) and the IMU selection of integrateUpToTime; adds slot k's frame as entry e
bool VIOFilterBatch::prepareFrame(int e, int k, double stamp, const eqvio_camera& cam, int M, const int* ids, const double* y, int* status) {
    status[e] = 0;
    if (k < 0 || k >= (int)slotv.size()) {
        status[e] = EQF_E_BAD_ARG;
        return false;
    }
    Slot& sl = slotv[k];
    if (stamp <= sl.currentTime || sl.currentTime < 0 || sl.velocityBuffer.empty() || !sl.initialised)
        return false;
    const size_t t = frames_.size();
    if (imus_.size() <= t)
        imus_.resize(t + 1), dts_.resize(t + 1), means_.resize(t + 1);
    const ImuSelection sel = selectImu(sl.velocityBuffer, sl.currentTime, stamp);
    means_[t].resize(13);
    sel.mean.pack(means_[t].data());
    imus_[t].resize(13 * sl.velocityBuffer.size());
    for (size_t i = 0; i < sl.velocityBuffer.size(); ++i)
        sl.velocityBuffer[i].pack(imus_[t].data() + 13 * i);
    dts_[t] = sel.dts;
    eqf_batch_frame f;
    f.slot = k;
    f.cam = cam;
    f.dt_total = sel.total;
    f.k = (int)sl.velocityBuffer.size();
    f.M = M;
    f.ids = ids;
    f.y = y;
    frames_.push_back(f);
    entry_.push_back(e);
    return true;
}
void VIOFilterBatch::stepPrepared(const int* slots, const double* stamps, int* status) {
    if (frames_.empty())
        return;
    for (size_t t = 0; t < frames_.size(); ++t) { // the vectors have their final addresses now
        frames_[t].imu13_mean = means_[t].data();
        frames_[t].imu13_k = imus_[t].data();
        frames_[t].dt_k = dts_[t].data();
    }
    st_.resize(frames_.size());
    // every listed slot to the call of its mode, in the order fast, accurate, discrete, and within a mode the Normal-chart slots behind the others: one device
    // call per (mode, Normal or not) group that is present - a step whose slots agree is one device call
    const auto call = [&](int which, int n, const eqf_batch_frame* fr, int* st) {
        if (which == 2)
            check(eqf_batch_step_discrete(batch, n, fr, st), "eqf_batch_step_discrete");
        else if (which == 1)
            check(eqf_batch_step_accurate(batch, n, fr, st), "eqf_batch_step_accurate");
        else
            check(eqf_batch_step(batch, n, fr, st), "eqf_batch_step");
    };
    bool mixed = false;
    const int group0 = groupOf(frames_[0].slot);
    for (size_t t = 1; t < frames_.size() && !mixed; ++t)
        mixed = groupOf(frames_[t].slot) != group0;
    if (!mixed) {
        call(callOf(frames_[0].slot), (int)frames_.size(), frames_.data(), st_.data());
    } else {
        std::vector<int> pst;
        for (int group = 0; group < 6; ++group) {
            const int which = group / 2;
            part_.clear(), partOf_.clear();
            for (size_t t = 0; t < frames_.size(); ++t)
                if (groupOf(frames_[t].slot) == group) {
                    part_.push_back(frames_[t]);
                    partOf_.push_back(t);
                }
            if (part_.empty())
                continue;
            pst.assign(part_.size(), 0);
            call(which, (int)part_.size(), part_.data(), pst.data());
            for (size_t t = 0; t < part_.size(); ++t)
                st_[partOf_[t]] = pst[t];
        }
    }
    for (size_t t = 0; t < frames_.size(); ++t) {
        const int e = entry_[t];
        status[e] = st_[t];
        if (st_[t] == EQF_E_BAD_ARG || st_[t] == EQF_E_CAPACITY)
            continue; // refused before the launch: the slot, its time and its IMU buffer are untouched
        Slot& sl = slotv[slots[e]];
        sl.currentTime = stamps[e];
        trimImuBuffer(sl.velocityBuffer, sl.currentTime);
    }
}
void VIOFilterBatch::processVisionData(int count, const int* slots, const double* stamps, const eqvio_camera* cams, const int* meas_counts, const int* ids_all,
                                       const double* y_all, int* status) {
    frames_.clear(), entry_.clear();
    size_t mo = 0;
    for (int e = 0; e < count; ++e) {
        prepareFrame(e, slots[e], stamps[e], cams[e], meas_counts[e], ids_all + mo, y_all + 2 * mo, status);
        mo += meas_counts[e];
    }
    stepPrepared(slots, stamps, status);
}
// getFeaturePredictions (VIOFilter.cpp:247-252) of every listed slot: the (sample, dt) lists of predictState from the slots' own buffers and times, then ONE
// eqf_batch_predictions call for the slots whose settings have useFeaturePredictions on
int VIOFilterBatch::getFeaturePredictions(int count, const int* slots, const eqvio_camera* cams, const double* stamps, eqf_batch_prediction_record* out, int* status) {
    std::vector<eqf_batch_prediction_entry> entries;
    std::vector<int> entryOf;
    std::vector<std::vector<double>> imus, dts;
    std::vector<char> listed(slotv.size(), 0);
    entries.reserve(count), entryOf.reserve(count), imus.reserve(count), dts.reserve(count);
    for (int e = 0; e < count; ++e) {
        const int k = slots[e];
        status[e] = 0;
        if (k < 0 || k >= (int)slotv.size() || listed[k]) {
            status[e] = EQF_E_BAD_ARG;
            continue;
        }
        listed[k] = 1;
        if (!slotSettings(k).useFeaturePredictions) { // the reference's empty measurement: nothing goes to the device
            std::memset(&out[e], 0, sizeof(out[e]));
            check(eqf_batch_sensor_estimate(batch, k, out[e].sensor), "eqf_batch_sensor_estimate");
            continue;
        }
        const Slot& sl = slotv[k];
        dts.push_back(imuDts(sl.velocityBuffer, sl.currentTime, stamps[e]));
        imus.emplace_back(13 * sl.velocityBuffer.size());
        for (size_t i = 0; i < sl.velocityBuffer.size(); ++i)
            sl.velocityBuffer[i].pack(imus.back().data() + 13 * i);
        entries.push_back(eqf_batch_prediction_entry{k, cams[e], (int)sl.velocityBuffer.size(), imus.back().data(), dts.back().data()});
        entryOf.push_back(e);
    }
    const int n = (int)entries.size();
    if (n == 0)
        return 0;
    if (n == count) // every entry goes: the records and codes land where the caller wants them
        return eqf_batch_predictions(batch, n, entries.data(), out, status);
    std::vector<eqf_batch_prediction_record> rec(n);
    std::vector<int> st(n, 0);
    if (const int rc = eqf_batch_predictions(batch, n, entries.data(), rec.data(), st.data()))
        return rc;
    for (int t = 0; t < n; ++t) {
        status[entryOf[t]] = st[t];
        if (st[t] == 0)
            out[entryOf[t]] = rec[t];
    }
    return 0;
}
void VIOFilterBatch::processVisionData(int count, const int* slots, const VisionMeasurement* const* meas, int* status) {
    frames_.clear(), entry_.clear();
    std::vector<double> stamps(count);
    for (int e = 0; e < count; ++e) {
        const VisionMeasurement& m = *meas[e];
        const auto fl = m.flat(); // validated against the measurement's map
        stamps[e] = m.stamp;
        prepareFrame(e, slots[e], m.stamp, m.cameraPtr->c, (int)fl.first->size(), fl.first->data(), fl.second->data(), status);
    }
    stepPrepared(slots, stamps.data(), status);
}

} // namespace eqvio_amd

// ------------------------------------------------------------------------------------------------ C-ABI
using eqvio_amd::IMUVelocity;
using eqvio_amd::VIOFilterBatch;
struct eqvio_batch {
    VIOFilterBatch* f = nullptr;
    std::string err;
    ~eqvio_batch() { delete f; }
};
namespace {
template <typename Fn> int guarded(eqvio_batch* b, Fn&& fn) {
    if (!b)
        return -1;
    try {
        fn();
        return 0;
    } catch (const std::exception& e) {
        b->err = e.what();
        return -1;
    }
}
bool slot_ok(const eqvio_batch* b, int k) { return b && k >= 0 && k < b->f->slots(); }
IMUVelocity imu_from13(const double* imu13) {
    IMUVelocity r;
    r.stamp = imu13[0];
    r.gyr = eqf::V3{imu13[1], imu13[2], imu13[3]};
    r.acc = eqf::V3{imu13[4], imu13[5], imu13[6]};
    r.gyrBiasVel = eqf::V3{imu13[7], imu13[8], imu13[9]};
    r.accBiasVel = eqf::V3{imu13[10], imu13[11], imu13[12]};
    return r;
}
} // namespace

int eqvio_batch_create(eqvio_batch** out, const eqvio_settings* s, int device, int slots, int max_landmarks) {
    if (!out || !s)
        return EQF_E_BAD_ARG;
    *out = nullptr;
    // the checks of eqf_batch_create, before anything touches a device: the sizes, then the settings
    if (slots < 1 || max_landmarks < 1 || max_landmarks > EQF_BATCH_MAX_LANDMARKS || device < 0)
        return EQF_E_BAD_ARG;
    if (const int rc = eqf_batch_check_settings(s))
        return rc;
    eqf_batch* core = nullptr;
    const int rc = eqf_batch_create(&core, device, slots, max_landmarks, s); // EQF_E_NO_DEVICE without a gfx950 device
    if (rc)
        return rc;
    auto* b = new eqvio_batch;
    try {
        b->f = new VIOFilterBatch(core); // releases core itself if it throws
    } catch (const eqvio_amd::BatchFailure& e) {
        delete b;
        return e.code;
    }
    *out = b;
    return 0;
}
int eqvio_batch_create_slot_from_state(eqvio_batch* b, int slot, const double* sensor, const int* ids, const double* p, int N, double time) {
    if (!slot_ok(b, slot) || !sensor || N < 0 || (N > 0 && (!ids || !p)))
        return EQF_E_BAD_ARG;
    return guarded(b, [&] { b->f->startFromState(slot, sensor, ids, p, N, time); });
}
void eqvio_batch_destroy(eqvio_batch* b) { delete b; }
const char* eqvio_batch_last_error(const eqvio_batch* b) { return b ? b->err.c_str() : "null batch"; }
int eqvio_batch_slots(const eqvio_batch* b) { return b ? b->f->slots() : EQF_E_BAD_ARG; }
int eqvio_batch_process_imu(eqvio_batch* b, int slot, const double* imu13) {
    if (!slot_ok(b, slot) || !imu13)
        return EQF_E_BAD_ARG;
    return guarded(b, [&] { b->f->processIMUData(slot, imu_from13(imu13)); });
}
int eqvio_batch_process_vision(eqvio_batch* b, int count, const int* slots, const double* stamps, const eqvio_camera* cams, const int* meas_counts, const int* ids_all,
                               const double* y_all, int* status) {
    if (!b || count < 0 || (count > 0 && (!slots || !stamps || !cams || !meas_counts || !status)))
        return EQF_E_BAD_ARG;
    return guarded(b, [&] { b->f->processVisionData(count, slots, stamps, cams, meas_counts, ids_all, y_all, status); });
}
int eqvio_batch_state_estimate(eqvio_batch* b, int slot, double* sensor, int* ids, double* p, int cap) {
    return slot_ok(b, slot) ? eqf_batch_state_estimate(b->f->core(), slot, sensor, ids, p, cap) : EQF_E_BAD_ARG;
}
int eqvio_batch_get_eqf(eqvio_batch* b, int slot, double* xi0_sensor, double* X_sensor, int* ids, double* q0, double* Q, int cap) {
    return slot_ok(b, slot) ? eqf_batch_get_state(b->f->core(), slot, xi0_sensor, X_sensor, ids, q0, Q, cap) : EQF_E_BAD_ARG;
}
int eqvio_batch_force_eqf(eqvio_batch* b, int slot, const double* xi0_sensor, const double* X_sensor, const int* ids, const double* q0, const double* Q, int N,
                          const double* sigma) {
    if (!slot_ok(b, slot) || !sigma)
        return EQF_E_BAD_ARG;
    const int rc = eqf_batch_set_state(b->f->core(), slot, xi0_sensor, X_sensor, ids, q0, Q, N);
    return rc ? rc : eqf_batch_set_sigma(b->f->core(), slot, sigma, 21 + 3 * N);
}
int eqvio_batch_sigma_dim(const eqvio_batch* b, int slot) { return slot_ok(b, slot) ? 21 + 3 * eqf_batch_num_landmarks(b->f->core(), slot) : EQF_E_BAD_ARG; }
int eqvio_batch_get_sigma(eqvio_batch* b, int slot, double* out, int n) { return slot_ok(b, slot) ? eqf_batch_get_sigma(b->f->core(), slot, out, n) : EQF_E_BAD_ARG; }
double eqvio_batch_get_time(const eqvio_batch* b, int slot) { return slot_ok(b, slot) ? b->f->slot(slot).currentTime : -1.0; }
int eqvio_batch_is_initialised(const eqvio_batch* b, int slot) { return slot_ok(b, slot) ? (b->f->slot(slot).initialised ? 1 : 0) : EQF_E_BAD_ARG; }
eqf_batch* eqvio_batch_core(eqvio_batch* b) { return b ? b->f->core() : nullptr; }
int eqvio_batch_set_slot_settings(eqvio_batch* b, int slot, const eqvio_settings* s) {
    if (!b || !s)
        return EQF_E_BAD_ARG;
    int code = 0;
    const int rc = guarded(b, [&] { code = b->f->setSlotSettings(slot, *s); }); // the checks are eqf_batch_set_slot_settings's
    return rc ? rc : code;
}
int eqvio_batch_set_slot_riccati(eqvio_batch* b, int slot, int mode) { return b ? b->f->setRiccatiMode(slot, mode) : EQF_E_BAD_ARG; }
int eqvio_batch_get_slot_riccati(const eqvio_batch* b, int slot) { return b ? b->f->riccatiMode(slot) : EQF_E_BAD_ARG; }
int eqvio_batch_set_slot_state_matrix(eqvio_batch* b, int slot, int kind) { return b ? b->f->setStateMatrix(slot, kind) : EQF_E_BAD_ARG; }
int eqvio_batch_get_slot_state_matrix(const eqvio_batch* b, int slot) { return b ? b->f->stateMatrix(slot) : EQF_E_BAD_ARG; }
int eqvio_batch_set_slot_chart(eqvio_batch* b, int slot, int chart) { return b ? b->f->setChart(slot, chart) : EQF_E_BAD_ARG; }
int eqvio_batch_get_slot_chart(const eqvio_batch* b, int slot) { return b ? b->f->chart(slot) : EQF_E_BAD_ARG; }
int eqvio_batch_convert_chart(eqvio_batch* b, int count, const int* slots, const int* charts, int* status) {
    if (!b || count < 0 || !slots || !charts || !status)
        return EQF_E_BAD_ARG;
    int code = 0;
    const int rc = guarded(b, [&] { code = b->f->convertChart(count, slots, charts, status); });
    return rc ? rc : code;
}
int eqvio_batch_get_slot_settings(const eqvio_batch* b, int slot, eqvio_settings* out) {
    return b ? eqf_batch_get_slot_settings(b->f->core(), slot, out) : EQF_E_BAD_ARG;
}
int eqvio_batch_last_innovation(const eqvio_batch* b, int slot, int* dof, double* nis, double* logdet) {
    return b ? eqf_batch_last_innovation(b->f->core(), slot, dof, nis, logdet) : EQF_E_BAD_ARG;
}
int eqvio_batch_innovation_totals(const eqvio_batch* b, int slot, long* updates, long* dof, double* nis, double* logdet) {
    return b ? eqf_batch_innovation_totals(b->f->core(), slot, updates, dof, nis, logdet) : EQF_E_BAD_ARG;
}
int eqvio_batch_reset_innovation_totals(eqvio_batch* b, int slot) { return b ? eqf_batch_reset_innovation_totals(b->f->core(), slot) : EQF_E_BAD_ARG; }
int eqvio_batch_copy_slots(eqvio_batch* b, int count, const int* src, const int* dst, int* status) {
    if (!b || count < 0 || !src || !dst || !status)
        return EQF_E_BAD_ARG;
    return guarded(b, [&] { b->f->copySlots(count, src, dst, status); });
}
int eqvio_batch_load_filter(eqvio_batch* b, eqvio_filter* src, int count, const int* slots, int* status) {
    if (!b || !src || count < 0 || !slots || !status)
        return EQF_E_BAD_ARG;
    int code = 0;
    const int rc = guarded(b, [&] { code = b->f->loadFilter(*eqvio_amd::filterOf(src), count, slots, status); });
    return rc ? rc : code;
}
int eqvio_batch_store_filter(eqvio_batch* b, int slot, eqvio_filter* dst) {
    if (!slot_ok(b, slot) || !dst)
        return EQF_E_BAD_ARG;
    int code = 0;
    const int rc = guarded(b, [&] { code = b->f->storeFilter(slot, *eqvio_amd::filterOf(dst)); });
    return rc ? rc : code;
}
int eqvio_batch_feature_predictions(eqvio_batch* b, int count, const int* slots, const eqvio_camera* cams, const double* stamps, eqf_batch_prediction_record* out,
                                    int* status) {
    if (!b || count < 0 || !slots || !cams || !stamps || !out || !status)
        return EQF_E_BAD_ARG;
    int code = 0;
    const int rc = guarded(b, [&] { code = b->f->getFeaturePredictions(count, slots, cams, stamps, out, status); });
    return rc ? rc : code;
}
int eqvio_batch_estimates(eqvio_batch* b, int count, const int* slots, eqf_batch_estimate_record* out, double* times, int* status) {
    if (!b || count < 0 || !slots || !out || !status)
        return EQF_E_BAD_ARG;
    const int rc = eqf_batch_estimates(b->f->core(), count, slots, out, status);
    for (int e = 0; e < count && rc == 0 && times; ++e)
        times[e] = eqvio_batch_get_time(b, slots[e]); // -1 for a slot that has not initialised (and for a refused index)
    return rc;
}

namespace {
// eqvio_batch_run_prepared (output_dir null) and eqvio_batch_run_prepared_recorded: one loop; the recorded one reads the estimates of the slots that had a
// frame after every step (eqf_batch_estimates is read-only, so the slots end in the same state bit for bit) and writes their rows
int run_prepared_loop(eqvio_batch* b, const eqvio_frames* const* per_slot, int first, int count, const char* output_dir) {
    const int B = b->f->slots();
    int steps = 0;
    const int rc = guarded(b, [&] {
        std::vector<std::unique_ptr<eqvio_amd::VIOWriter>> writers(B); // output_dir/run_<k>/ of every slot with a sequence, before any frame runs
        for (int k = 0; k < B && output_dir; ++k)
            if (per_slot[k])
                writers[k] = eqvio_amd::makeRunWriter(output_dir, k);
        std::vector<eqf_batch_estimate_record> rec;
        std::vector<int> slots, status;
        std::vector<const eqvio_amd::VisionMeasurement*> meas;
        slots.reserve(B), status.reserve(B), meas.reserve(B);
        for (int j = first; j < first + count; ++j) {
            slots.clear(), meas.clear();
            for (int k = 0; k < B; ++k) {
                const eqvio_frames* fr = per_slot[k];
                if (!fr || j >= (int)fr->meas.size())
                    continue; // this slot's sequence has ended (or it has none): it sits the step out
                for (size_t s = fr->imuBegin[j]; s < fr->imuBegin[j + 1]; ++s)
                    b->f->processIMUData(k, fr->imus[s]);
                slots.push_back(k);
                meas.push_back(&fr->meas[j]);
            }
            if (slots.empty())
                break;
            status.assign(slots.size(), 0);
            b->f->processVisionData((int)slots.size(), slots.data(), meas.data(), status.data());
            for (size_t e = 0; e < slots.size(); ++e)
                if (status[e] != 0)
                    throw std::runtime_error("frame " + std::to_string(j) + ", slot " + std::to_string(slots[e]) + ": " + eqf_error_string(status[e]));
            if (output_dir) {
                rec.resize(slots.size());
                eqvio_amd::check(eqf_batch_estimates(b->f->core(), (int)slots.size(), slots.data(), rec.data(), status.data()), "eqf_batch_estimates");
                for (size_t e = 0; e < slots.size(); ++e) {
                    if (status[e] != 0)
                        throw std::runtime_error("estimates, frame " + std::to_string(j) + ", slot " + std::to_string(slots[e]) + ": " + eqf_error_string(status[e]));
                    eqvio_amd::writeEstimateRecord(*writers[slots[e]], b->f->slot(slots[e]).currentTime, rec[e]);
                }
            }
            ++steps;
        }
    });
    return rc ? rc : steps;
}
} // namespace
int eqvio_batch_run_prepared(eqvio_batch* b, const eqvio_frames* const* per_slot, int first, int count) {
    if (!b || !per_slot || first < 0 || count < 0)
        return EQF_E_BAD_ARG;
    return run_prepared_loop(b, per_slot, first, count, nullptr);
}
int eqvio_batch_run_prepared_recorded(eqvio_batch* b, const eqvio_frames* const* per_slot, int first, int count, const char* output_dir) {
    if (!b || !per_slot || first < 0 || count < 0 || !output_dir)
        return EQF_E_BAD_ARG;
    return run_prepared_loop(b, per_slot, first, count, output_dir);
}

namespace {
// the entries of eqvio_batch_compute_nees / eqvio_batch_consistency as eqf_batch_truth
std::vector<eqf_batch_truth> truths_of(int count, const int* slots, const double* true_sensor_all, const int* true_counts, const int* true_ids_all, const double* true_p_all) {
    std::vector<eqf_batch_truth> t(count);
    size_t o = 0;
    for (int e = 0; e < count; ++e) {
        t[e].slot = slots[e];
        t[e].sensor = true_sensor_all + 23 * (size_t)e;
        t[e].n_true = true_counts[e];
        t[e].ids = true_ids_all ? true_ids_all + o : nullptr;
        t[e].p = true_p_all ? true_p_all + 3 * o : nullptr;
        o += std::max(true_counts[e], 0);
    }
    return t;
}
} // namespace
int eqvio_batch_compute_nees(eqvio_batch* b, int count, const int* slots, const double* true_sensor_all, const int* true_counts, const int* true_ids_all,
                             const double* true_p_all, double* nees, int* status) {
    if (!b || count < 0 || (count > 0 && (!slots || !true_sensor_all || !true_counts || !nees || !status)))
        return EQF_E_BAD_ARG;
    return eqf_batch_nees(b->f->core(), count, truths_of(count, slots, true_sensor_all, true_counts, true_ids_all, true_p_all).data(), nees, status);
}
int eqvio_batch_consistency(eqvio_batch* b, int count, const int* slots, const double* true_sensor_all, const int* true_counts, const int* true_ids_all,
                            const double* true_p_all, eqf_batch_consistency_record* out, int* status) {
    if (!b || count < 0 || (count > 0 && (!slots || !true_sensor_all || !true_counts || !out || !status)))
        return EQF_E_BAD_ARG;
    return eqf_batch_consistency(b->f->core(), count, truths_of(count, slots, true_sensor_all, true_counts, true_ids_all, true_p_all).data(), out, status);
}
int eqvio_batch_augment_landmark_states(eqvio_batch* b, int count, const int* slots, const int* new_counts, const int* new_ids_all, const int* prov_counts,
                                        const int* prov_ids_all, const double* prov_p_all, int* status) {
    if (!b || count < 0 || (count > 0 && (!slots || !new_counts || !prov_counts || !status)))
        return EQF_E_BAD_ARG;
    std::vector<eqf_batch_augment_entry> a(count);
    size_t on = 0, op = 0;
    for (int e = 0; e < count; ++e) {
        a[e].slot = slots[e];
        a[e].n_new = new_counts[e];
        a[e].new_ids = new_ids_all ? new_ids_all + on : nullptr;
        a[e].n_prov = prov_counts[e];
        a[e].prov_ids = prov_ids_all ? prov_ids_all + op : nullptr;
        a[e].prov_p = prov_p_all ? prov_p_all + 3 * op : nullptr;
        on += std::max(new_counts[e], 0);
        op += std::max(prov_counts[e], 0);
    }
    return eqf_batch_augment(b->f->core(), count, a.data(), status);
}

namespace {
// eqvio_batch_run_sim (output_dir null) and eqvio_batch_run_sim_recorded: one loop, whose NEES call is eqf_batch_nees or eqf_batch_consistency
int run_sim_loop(eqvio_batch* b, eqvio_sim* const* sims, int max_frames, double* nees, int* frames_run, const char* output_dir) {
    *frames_run = 0;
    const int B = b->f->slots();
    for (size_t i = 0; i < (size_t)max_frames * B; ++i)
        nees[i] = std::nan("");
    return guarded(b, [&] {
        VIOFilterBatch& f = *b->f;
        std::vector<std::unique_ptr<eqvio_amd::VIOWriter>> writers(B); // output_dir/run_<k>/ of every slot with a sim, before any frame runs
        for (int k = 0; k < B && output_dir; ++k) {
            if (!sims[k])
                continue;
            const std::string dir = std::string(output_dir) + "/run_" + std::to_string(k);
            writers[k] = std::make_unique<eqvio_amd::VIOWriter>(dir);
            struct stat st;
            if (stat(dir.c_str(), &st) != 0 || !S_ISDIR(st.st_mode))
                throw std::runtime_error("cannot create the output directory " + dir);
        }
        std::vector<eqf_batch_consistency_record> rec;
        struct SimSlot {
            int np = 0, M = 0;
            bool image = false; // an image is in hand
            double stamp = 0, sensor[23];
            std::vector<int> tids, ids;
            std::vector<double> tp, y;
            eqvio_camera cam;
        };
        std::vector<SimSlot> ss(B);
        // slot k's measurements up to its next image: the IMU samples go to the slot (or to `held`); false at the end of the sequence
        auto next_image = [&](int k, std::vector<IMUVelocity>* held) {
            SimSlot& s = ss[k];
            for (;;) {
                const int type = eqvio_sim_next_measurement_type(sims[k]);
                if (type == EQVIO_MEAS_NONE)
                    return false;
                if (type == EQVIO_MEAS_IMAGE) {
                    s.M = eqvio_sim_get_vision(sims[k], &s.stamp, s.ids.data(), s.y.data(), s.np);
                    if (s.M < 0)
                        throw std::runtime_error("slot " + std::to_string(k) + ": more features than world points");
                    return true;
                }
                double imu[13];
                eqvio_sim_get_imu(sims[k], imu);
                if (held)
                    held->push_back(imu_from13(imu));
                else
                    f.processIMUData(k, imu_from13(imu));
            }
        };
        auto truth = [&](int k, double stamp, int noise) {
            SimSlot& s = ss[k];
            if (eqvio_sim_true_state(sims[k], stamp, noise, s.sensor, s.tids.data(), s.tp.data(), s.np) != s.np)
                throw std::runtime_error("eqvio_sim_true_state");
        };
        // start: getInitialCondition() (main_sim.cpp:105) trimmed to the first image's ids, in the initial condition's order
        for (int k = 0; k < B; ++k) {
            if (!sims[k])
                continue;
            SimSlot& s = ss[k];
            s.np = eqvio_sim_num_points(sims[k]);
            s.tids.resize(s.np + 1), s.tp.resize(3 * (size_t)s.np + 3), s.ids.resize(s.np + 1), s.y.resize(2 * (size_t)s.np + 2);
            eqvio_sim_camera(sims[k], &s.cam);
            truth(k, 0.0, 1);
            std::vector<double> s0(s.sensor, s.sensor + 23);
            std::vector<IMUVelocity> held;
            s.image = next_image(k, &held);
            std::vector<int> ids;
            std::vector<double> p;
            for (int i = 0; i < s.np && s.image; ++i)
                if (std::binary_search(s.ids.begin(), s.ids.begin() + s.M, s.tids[i])) {
                    ids.push_back(s.tids[i]);
                    p.insert(p.end(), s.tp.begin() + 3 * i, s.tp.begin() + 3 * i + 3);
                }
            f.startFromState(k, s0.data(), ids.data(), p.data(), (int)ids.size(), 0.0);
            for (const IMUVelocity& u : held)
                f.processIMUData(k, u);
        }
        std::vector<int> slots, status, counts, ids_all, tcounts, tids_all;
        std::vector<double> stamps, y_all, sensors, tp_all, out;
        std::vector<eqvio_camera> cams;
        std::vector<eqf_batch_augment_entry> aug;
        std::vector<eqf_batch_truth> tr;
        auto fail = [&](const char* what, size_t e, int code) {
            throw std::runtime_error(std::string(what) + ", frame " + std::to_string(*frames_run) + ", slot " + std::to_string(slots[e]) + ": " + eqf_error_string(code));
        };
        while (*frames_run < max_frames) {
            slots.clear();
            for (int k = 0; k < B; ++k)
                if (sims[k] && ss[k].image)
                    slots.push_back(k);
            if (slots.empty())
                break;
            const size_t n = slots.size();
            // augmentLandmarkStates(ids, getTrueState(stamp, true)) (main_sim.cpp:137-140)
            aug.resize(n), status.assign(n, 0);
            for (size_t e = 0; e < n; ++e) {
                SimSlot& s = ss[slots[e]];
                truth(slots[e], s.stamp, 1);
                aug[e] = eqf_batch_augment_entry{slots[e], s.M, s.ids.data(), s.np, s.tids.data(), s.tp.data()};
            }
            eqvio_amd::check(eqf_batch_augment(f.core(), (int)n, aug.data(), status.data()), "eqf_batch_augment");
            for (size_t e = 0; e < n; ++e)
                if (status[e])
                    fail("augment", e, status[e]);
            // processVisionData
            stamps.clear(), cams.clear(), counts.clear(), ids_all.clear(), y_all.clear();
            for (int k : slots) {
                const SimSlot& s = ss[k];
                stamps.push_back(s.stamp);
                cams.push_back(s.cam);
                counts.push_back(s.M);
                ids_all.insert(ids_all.end(), s.ids.begin(), s.ids.begin() + s.M);
                y_all.insert(y_all.end(), s.y.begin(), s.y.begin() + 2 * s.M);
            }
            f.processVisionData((int)n, slots.data(), stamps.data(), cams.data(), counts.data(), ids_all.data(), y_all.data(), status.data());
            for (size_t e = 0; e < n; ++e)
                if (status[e])
                    fail("vision", e, status[e]);
            // computeNEES(getTrueState(getTime())) (main_sim.cpp:145-147)
            tr.resize(n), out.resize(n);
            for (size_t e = 0; e < n; ++e) {
                SimSlot& s = ss[slots[e]];
                truth(slots[e], f.slot(slots[e]).currentTime, 0);
                tr[e] = eqf_batch_truth{slots[e], s.sensor, s.np, s.tids.data(), s.tp.data()};
            }
            if (output_dir) {
                rec.resize(n);
                eqvio_amd::check(eqf_batch_consistency(f.core(), (int)n, tr.data(), rec.data(), status.data()), "eqf_batch_consistency");
            } else
                eqvio_amd::check(eqf_batch_nees(f.core(), (int)n, tr.data(), out.data(), status.data()), "eqf_batch_nees");
            for (size_t e = 0; e < n; ++e) {
                if (status[e])
                    fail("nees", e, status[e]);
                nees[(size_t)*frames_run * B + slots[e]] = output_dir ? rec[e].nees : out[e];
                if (output_dir)
                    eqvio_amd::writeConsistencyRecord(*writers[slots[e]], f.slot(slots[e]).currentTime, rec[e], ss[slots[e]].np, ss[slots[e]].tids.data());
            }
            ++*frames_run;
            for (int k : slots)
                ss[k].image = next_image(k, nullptr);
        }
    });
}
} // namespace
int eqvio_batch_run_sim(eqvio_batch* b, eqvio_sim* const* sims, int max_frames, double* nees, int* frames_run) {
    if (!b || !sims || max_frames < 0 || (max_frames > 0 && !nees) || !frames_run)
        return EQF_E_BAD_ARG;
    return run_sim_loop(b, sims, max_frames, nees, frames_run, nullptr);
}
int eqvio_batch_run_sim_recorded(eqvio_batch* b, eqvio_sim* const* sims, int max_frames, double* nees, int* frames_run, const char* output_dir) {
    if (!b || !sims || max_frames < 0 || (max_frames > 0 && !nees) || !frames_run || !output_dir)
        return EQF_E_BAD_ARG;
    return run_sim_loop(b, sims, max_frames, nees, frames_run, output_dir);
}
