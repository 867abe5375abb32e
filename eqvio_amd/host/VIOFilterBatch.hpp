// VIOFilterBatch: the batched counterpart of VIOFilter (VIOFilter.hpp) - B slots, each the host state of one reference VIOFilter (IMU buffer, current
// time, initialised flag; the EqF state lives in the device batch of include/eqf_batch.h), whose frames go to the device in one step.
#pragma once
#include "VIOFilter.hpp"
#include "VIOWriter.hpp"
#include "eqf_batch.h"
#include <memory>
#include <string>
#include <vector>

namespace eqvio_amd {

// IMU selection of VIOFilter::integrateUpToTime, fast-Riccati branch (src/VIOFilter.cpp:134-192): the dt of every buffered sample up to newTime, the mean
// sample of the Riccati step over their sum, and the samples the buffer keeps afterwards. Same expressions as VIOFilter.cpp's mirror.
struct ImuSelection {
    std::vector<double> dts;
    IMUVelocity mean;
    double total = 0;
};
// the dt of every buffered sample up to newTime: the loop integrateUpToTime and VIO_eqf::predictState (VIO_eqf.cpp:139-151) share
std::vector<double> imuDts(const std::vector<IMUVelocity>& buffer, double currentTime, double newTime);
ImuSelection selectImu(const std::vector<IMUVelocity>& buffer, double currentTime, double newTime);
void trimImuBuffer(std::vector<IMUVelocity>& buffer, double currentTime);

// One frame's rows of nees.csv, poseConsistency.csv, cameraConsistency.csv, biasConsistency.csv and landmarkError.csv from a slot's consistency record
// (eqf_batch_consistency), through VIOWriter's own row formatting: what writeConsistency and writeLandmarkError write for a single filter. landmarkError.csv
// has one column per TRUE landmark (true_ids, the true state's order), NaN where the slot does not hold it.
void writeConsistencyRecord(VIOWriter& writer, double stamp, const eqf_batch_consistency_record& record, int n_true, const int* true_ids);
// One frame's rows of IMUState.csv, camera.csv, bias.csv and points.csv from a slot's estimate record (eqf_batch_estimates), through VIOWriter's own row
// formatting: what writeStates writes for a single filter. points.csv takes the record's p_world.
void writeEstimateRecord(VIOWriter& writer, double stamp, const eqf_batch_estimate_record& record);
// output_dir/run_<k>/ as a VIOWriter whose four state files start anew: the directory is made, files of an earlier run are removed (a file appears with its
// first row). Throws when the directory cannot be created.
std::unique_ptr<VIOWriter> makeRunWriter(const std::string& output_dir, int k);

class VIOFilterBatch {
  public:
    struct Slot {
        std::vector<IMUVelocity> velocityBuffer;
        double currentTime = -1.0;
        bool initialised = false;
    };
    // takes ownership of a batch made by eqf_batch_create; the slots' settings are the device layer's (eqf_batch_get_slot_settings), kept nowhere else
    explicit VIOFilterBatch(eqf_batch* batch);
    ~VIOFilterBatch();
    VIOFilterBatch(const VIOFilterBatch&) = delete;
    VIOFilterBatch& operator=(const VIOFilterBatch&) = delete;
    // The slot's own settings, from its next frame on (eqf_batch_set_slot_settings; returns its code, and nothing changes unless that is 0). The
    // initial-value fields (cameraOffset, the initial sensor variances) only matter to a slot that has not initialised yet: when the call changes one of them
    // on such a slot, while it holds no landmark, the slot is put back to what VIOFilter(const Settings&) makes of the new settings - which replaces a state or
    // Sigma planted there through core(). Any other call, and any call on an initialised slot, keeps state and Sigma. If that reset fails on the device the
    // call throws and the slot has its former settings again.
    int setSlotSettings(int slot, const eqvio_settings& s);
    eqvio_settings slotSettings(int slot) const;
    // The propagation a slot's frames take (include/eqvio_batch.h): EQVIO_BATCH_RICCATI_FAST (eqf_batch_step; every slot starts with it) or _ACCURATE
    // (eqf_batch_step_accurate). slot < 0: every slot. Kept like the settings: copySlots and loadFilter leave the destination's mode alone. Returns 0 or
    // EQF_E_BAD_ARG (bad mode or slot; nothing changes); riccatiMode returns the mode or EQF_E_BAD_ARG.
    int setRiccatiMode(int slot, int mode);
    int riccatiMode(int slot) const;
    // The state matrix an ACCURATE slot's Riccati steps use, the reference's useDiscreteStateMatrix (include/eqvio_batch.h): EQVIO_BATCH_STATE_MATRIX_CONTINUOUS
    // (every slot starts with it) or _DISCRETE (eqf_batch_step_discrete). A fast slot ignores it. Kept and refused like the Riccati mode.
    int setStateMatrix(int slot, int kind);
    int stateMatrix(int slot) const;
    // The slot's coordinate chart on its own, the Normal chart included (eqf_batch_set_slot_chart, include/eqf_batch.h: the chart is the device layer's, kept
    // nowhere else). slot < 0: every slot - then nothing changes unless every slot takes the chart. Returns 0 or EQF_E_BAD_ARG (a chart outside the enum, a bad
    // slot, or a slot that holds landmarks under another chart); chart returns the slot's chart or EQF_E_BAD_ARG.
    int setChart(int slot, int chart);
    int chart(int slot) const;
    // Entry e: slot slots[e] is re-expressed in chart charts[e] while it holds landmarks, on the device (eqf_batch_convert_chart: one launch, same status codes
    // and refusals; Sigma <- T Sigma T^T). The host half (IMU buffer, time, flags) is not involved; the Riccati mode and the state-matrix choice are kept.
    // Returns eqf_batch_convert_chart's code.
    int convertChart(int count, const int* slots, const int* charts, int* status);
    // Entry e: slot dst[e] becomes slot src[e] as it was before the call - the EqF state on the device (eqf_batch_copy_slots: one launch, same status codes)
    // and the host half: IMU buffer, current time, initialised flag. The destination keeps its settings and innovation totals. A refused entry changes nothing.
    void copySlots(int count, const int* src, const int* dst, int* status);
    // Every listed slot becomes the filter: its EqF state on the device (eqf_batch_load_ctx: one launch for the whole call, same status codes; a whole-call
    // refusal is returned and nothing changes) and the host half copySlots moves - IMU buffer, current time, initialised flag. The destination keeps its own
    // settings and innovation totals; a refused entry changes nothing. The filter is unchanged (a removal of invalid landmarks it had deferred happens first).
    int loadFilter(VIOFilter& src, int count, const int* slots, int* status);
    // The filter becomes the slot (eqf_batch_store_ctx, then the host half); it keeps its own settings. Returns eqf_batch_store_ctx's code; nothing changes
    // unless that is 0.
    int storeFilter(int slot, VIOFilter& dst);
    void startFromState(int slot, const double* sensor, const int* ids, const double* p, int N, double time);
    void processIMUData(int slot, const IMUVelocity& imu);
    // processVisionData for `count` slots in one device step; status per entry
    void processVisionData(int count, const int* slots, const double* stamps, const eqvio_camera* cams, const int* meas_counts, const int* ids_all,
                           const double* y_all, int* status);
    // the same for measurements already built (a replay's VisionMeasurement objects): one device step for every listed slot
    void processVisionData(int count, const int* slots, const VisionMeasurement* const* meas, int* status);
    // getFeaturePredictions(cams[e], stamps[e]) (VIOFilter.cpp:247-252) of `count` distinct slots: each slot's state estimate pushed through its own buffered
    // IMU samples up to the stamp (predictState's dts from its velocityBuffer and currentTime) and projected, with the landmarks' output covariances, in ONE
    // eqf_batch_predictions call. A slot whose settings have useFeaturePredictions off gets the reference's empty measurement - N = 0, every array zero, sensor
    // its current estimate, status 0 - and is not sent to the device; a slot that has not initialised has no sample: its current estimate. status[e] 0 or
    // EQF_E_BAD_ARG (bad or repeated slot, bad camera: out[e] untouched). Nothing of any slot changes. Returns eqf_batch_predictions's code.
    int getFeaturePredictions(int count, const int* slots, const eqvio_camera* cams, const double* stamps, eqf_batch_prediction_record* out, int* status);
    // the innovation statistics of the slot's updated steps since the last reset (eqf_batch_innovation_totals: the numbers are the device batch's)
    struct InnovationTotals {
        long updates = 0, dof = 0;
        double nis = 0, logdet = 0;
        double meanNisPerDof() const { return nis / (double)dof; }
        double logLikelihood() const { return -0.5 * (nis + logdet + (double)dof * 1.8378770664093453); } // ln 2 pi
    };
    InnovationTotals innovationTotals(int slot) const;
    eqf_batch* core() { return batch; }
    const eqf_batch* core() const { return batch; }
    Slot& slot(int k) { return slotv.at(k); }
    const Slot& slot(int k) const { return slotv.at(k); }
    int slots() const { return (int)slotv.size(); }

  private:
    std::vector<eqf_batch_frame> frames_;
    std::vector<int> entry_, st_;
    std::vector<std::vector<double>> imus_, dts_, means_;
    bool prepareFrame(int e, int k, double stamp, const eqvio_camera& cam, int M, const int* ids, const double* y, int* status);
    void stepPrepared(const int* slots, const double* stamps, int* status);
    void initialiseFromIMUData(int slot, const IMUVelocity& imu);
    void resetSlot(int slot);
    eqf_batch* batch = nullptr;
    std::vector<Slot> slotv;
    std::vector<int> riccati_; // per slot: EQVIO_BATCH_RICCATI_*
    std::vector<int> stateMatrix_; // per slot: EQVIO_BATCH_STATE_MATRIX_*
    // the device call slot k's frames go to: 0 eqf_batch_step, 1 eqf_batch_step_accurate, 2 eqf_batch_step_discrete
    int callOf(int k) const;
    // the group of a step slot k's frame goes in: 2 callOf(k) + (the slot's chart is Normal) - one device call per group that is present
    int groupOf(int k) const;
    std::vector<eqf_batch_frame> part_; // stepPrepared: the frames of one mode
    std::vector<size_t> partOf_;
};

} // namespace eqvio_amd
