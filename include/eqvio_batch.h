/* eqvio_batch.h — C-ABI of the filter-level batch (eqvio_amd/host/VIOFilterBatch.hpp): B reference VIOFilters (fast or, per slot, accurate Riccati with the continuous or the discrete state matrix; <= 64
 * landmarks each) whose frames go to the device together, one device call per step and mode (include/eqf_batch.h). Each slot keeps what the reference's VIOFilter keeps on the host:
 * its IMU buffer, current time, initialised flag and landmark ids.
 *
 * Return values: 0 / a count on success, -1 when the C++ layer threw (message via eqvio_batch_last_error), an EQF_E_* code for refused arguments
 * (eqvio_batch_create checks them before it looks for a device, see eqf_batch_create).
 */
#ifndef EQVIO_BATCH_H
#define EQVIO_BATCH_H
#include "eqf_batch.h"
#include "eqvio_filter.h"
#include "eqvio_sim.h"
#include "eqvio_types.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct eqvio_batch eqvio_batch;

/* every slot as VIOFilter(const Settings&) (src/VIOFilter.cpp:31-41): it initialises itself from its first IMU sample. The settings are every slot's until
 * eqvio_batch_set_slot_settings gives a slot its own. */
int eqvio_batch_create(eqvio_batch** out, const eqvio_settings* settings, int device, int slots, int max_landmarks);
/* The slot's own settings (eqf_batch_set_slot_settings, include/eqf_batch.h: same refusals, same codes, the slot untouched when refused), from the slot's next
 * frame on; every other slot keeps its own. Whatever the host layer derives from settings uses the slot's copy. The initial-value fields (cameraOffset and the
 * initial*Variance fields) only matter to a slot that has not initialised yet: a call that changes one of them on such a slot, while it holds no landmark, puts
 * the slot back to what VIOFilter(const Settings&) makes of the new settings (this replaces a state or Sigma planted there through eqvio_batch_core), and
 * eqvio_batch_create_slot_from_state takes its initial covariance from them; every other call, and every call on a slot that has initialised, keeps state and
 * Sigma, and only the filter parameters change. Nothing changes unless the return value is 0: if that reset fails on the device (-1, eqvio_batch_last_error) the
 * slot has its former settings again. eqvio_batch_run_prepared / _run_sim with the same sequence or simulator seed in
 * every slot, after per-slot settings were set, is a settings sweep. get returns the slot's settings. */
int eqvio_batch_set_slot_settings(eqvio_batch* b, int slot, const eqvio_settings* settings);
int eqvio_batch_get_slot_settings(const eqvio_batch* b, int slot, eqvio_settings* out);
/* The propagation a slot's frames take: EQVIO_BATCH_RICCATI_FAST - eqf_batch_step, one integrateRiccatiStateFast per frame; every slot starts with it - or
 * EQVIO_BATCH_RICCATI_ACCURATE - eqf_batch_step_accurate, the reference's default (fastRiccati: false): one integrateRiccatiStateAccurate per IMU sample,
 * between the observer steps. As in the reference's layering (VIO_eqf offers both integrations, the filter above picks one) the mode is not a setting: a batch's
 * settings keep saying fastRiccati = 1, which describes eqf_batch_step. eqvio_batch_process_vision, _run_prepared(_recorded) and _run_sim(_recorded) send every
 * step's listed slots to the call of their mode; a step that lists slots of both modes makes two device calls, the fast slots first. set: slot < 0 means every
 * slot; a mode outside the enum, a slot index past the last slot or a null batch gives EQF_E_BAD_ARG, nothing changed, no device looked at. get returns the mode,
 * or EQF_E_BAD_ARG. The mode is kept like the settings: eqvio_batch_copy_slots and _load_filter leave the destination's mode alone, _store_filter leaves the
 * filter's settings alone. */
enum { EQVIO_BATCH_RICCATI_FAST = 0, EQVIO_BATCH_RICCATI_ACCURATE = 1 };
int eqvio_batch_set_slot_riccati(eqvio_batch* b, int slot, int mode); /* slot < 0: every slot */
int eqvio_batch_get_slot_riccati(const eqvio_batch* b, int slot);     /* mode, or EQF_E_BAD_ARG */
/* The state matrix an ACCURATE slot's Riccati steps use - the reference picks its propagation with two booleans, fastRiccati and useDiscreteStateMatrix
 * (integrateUpToTime, src/VIOFilter.cpp:160-178), and this is the second one: EQVIO_BATCH_STATE_MATRIX_CONTINUOUS - eqf_batch_step_accurate; every slot starts
 * with it - or EQVIO_BATCH_STATE_MATRIX_DISCRETE - eqf_batch_step_discrete, one integrateRiccatiStateDiscrete per IMU sample (A_d = stateMatrixADiscrete, the
 * mode the reference's own statistical test runs). The choice matters only while the slot's Riccati mode is EQVIO_BATCH_RICCATI_ACCURATE, as in
 * integrateUpToTime; a fast slot keeps it and ignores it. Like the Riccati mode it is not a setting: the useDiscreteStateMatrix field of eqvio_settings is not read
 * by the batch. A step sends its listed slots to the calls of their modes in the order fast, accurate, discrete: one device call when the slots agree, up to
 * three when they do not. set: slot < 0 means every slot; a kind outside the enum, a slot index past the last slot or a null batch gives EQF_E_BAD_ARG, nothing
 * changed, no device looked at. get returns the kind, or EQF_E_BAD_ARG. Kept like the Riccati mode: eqvio_batch_copy_slots and _load_filter leave the
 * destination's choice alone, _store_filter leaves the filter's settings alone. */
enum { EQVIO_BATCH_STATE_MATRIX_CONTINUOUS = 0, EQVIO_BATCH_STATE_MATRIX_DISCRETE = 1 };
int eqvio_batch_set_slot_state_matrix(eqvio_batch* b, int slot, int kind); /* slot < 0: every slot */
int eqvio_batch_get_slot_state_matrix(const eqvio_batch* b, int slot);     /* kind, or EQF_E_BAD_ARG */
/* The slot's coordinate chart on its own: EQVIO_COORD_EUCLIDEAN, EQVIO_COORD_INVDEPTH or EQVIO_COORD_NORMAL (eqf_batch_set_slot_chart, include/eqf_batch.h) -
 * the way to the reference's third chart, which eqvio_batch_create and eqvio_batch_set_slot_settings keep refusing in the settings. From the slot's next frame
 * on; eqvio_batch_get_slot_settings then reports it in coordinateChoice, and a later accepted eqvio_batch_set_slot_settings replaces it with its own. A step
 * whose slots mix charts and modes makes one device call per (mode, Normal or not) group that is present, in the order fast, accurate, discrete and the Normal
 * slots of a mode behind its others. set: slot < 0 means every slot, and then nothing changes unless every slot takes the chart; a chart outside the enum, a
 * slot index past the last slot, a null batch, or a slot that holds landmarks under another chart (its Sigma is in that chart's coordinates) gives
 * EQF_E_BAD_ARG, nothing changed, no device looked at. get returns the chart, or EQF_E_BAD_ARG. eqvio_batch_load_filter / _store_filter keep refusing a
 * Normal-chart filter (eqf_batch_load_ctx / _store_ctx). eqvio_batch_convert_chart changes the chart of a slot that holds landmarks, Sigma with it. */
int eqvio_batch_set_slot_chart(eqvio_batch* b, int slot, int chart); /* slot < 0: every slot */
int eqvio_batch_get_slot_chart(const eqvio_batch* b, int slot);     /* chart, or EQF_E_BAD_ARG */
/* Changes the chart of slots that hold landmarks (eqf_batch_convert_chart, include/eqf_batch.h: one launch, Sigma <- T Sigma T^T on the device, the same
 * per-entry status codes and refusals): entry e re-expresses slot slots[e] in chart charts[e]. It is the same filter, described differently: the state, the
 * ids, every other setting, the Riccati mode, the state-matrix choice, the innovation totals and the last result are kept, and the host half of the slot (IMU
 * buffer, current time, initialised flag) is not involved. To warm up once, eqvio_batch_copy_slots into B slots and branch into the three charts from the same
 * belief. Returns 0 when it ran (whatever the per-entry codes), EQF_E_BAD_ARG (a null batch, slots, charts or status, count < 0; no device is looked at) or a
 * HIP error. */
int eqvio_batch_convert_chart(eqvio_batch* b, int count, const int* slots, const int* charts, int* status);
/* slot starts as VIOFilter(const VIOState&, const Settings&, time) (VIOFilter.cpp:43-56), with the slot's settings */
int eqvio_batch_create_slot_from_state(eqvio_batch* b, int slot, const double* sensor, const int* ids, const double* p, int N, double time);
void eqvio_batch_destroy(eqvio_batch* b);
const char* eqvio_batch_last_error(const eqvio_batch* b);
int eqvio_batch_slots(const eqvio_batch* b);

/* processIMUData (VIOFilter.cpp:58-63) of one slot */
int eqvio_batch_process_imu(eqvio_batch* b, int slot, const double* imu13);
/* processVisionData (VIOFilter.cpp:194-241) of `count` distinct slots in ONE device step. Entry e: slot slots[e], stamp stamps[e], camera cams[e],
 * meas_counts[e] features (ids ascending) taken in order from ids_all / y_all. A slot whose frame the reference would skip (stale stamp, no IMU yet, not
 * initialised) sits the step out with status 0. status[e]: 0 or the slot's EQF_E_* code (include/eqf_batch.h). Returns 0 or -1. */
int eqvio_batch_process_vision(eqvio_batch* b, int count, const int* slots, const double* stamps, const eqvio_camera* cams, const int* meas_counts, const int* ids_all,
                               const double* y_all, int* status);

/* Lockstep replay of prepared sequences (eqvio_frames_create, include/eqvio_filter.h): per_slot[k] is slot k's sequence or NULL. For j in [first, first + count)
 * frame j of every slot that has one - its IMU samples, then its measurement - goes in one device step; a slot whose sequence has ended sits out. Returns the
 * number of steps run, or -1 (a slot's frame was refused or failed: message via eqvio_batch_last_error). */
int eqvio_batch_run_prepared(eqvio_batch* b, const eqvio_frames* const* per_slot, int first, int count);
/* eqvio_batch_run_prepared with the estimates recorded: the same loop with the same steps, leaving every slot in the same state bit for bit, and after every
 * step ONE eqf_batch_estimates call for the slots that had a frame. For every slot k with a sequence the directory output_dir/run_<k>/ gets IMUState.csv,
 * camera.csv, bias.csv and points.csv with the headers, column order and number formatting of a single filter's --output (VIOWriter::writeStates): one row per
 * frame the slot ran, stamp = the slot's getTime(); points.csv takes the records' p_world. Each call starts its files anew (files of an earlier call are
 * removed), and a file appears with its first row. Only the records cross to the host. An output_dir that cannot be created gives -1
 * (eqvio_batch_last_error) before any frame runs; a null one EQF_E_BAD_ARG. */
int eqvio_batch_run_prepared_recorded(eqvio_batch* b, const eqvio_frames* const* per_slot, int first, int count, const char* output_dir);

/* viewEqFState().computeNEES(trueState) of `count` distinct slots in ONE launch (eqf_batch_nees). Entry e: slot slots[e], the 23 sensor doubles at
 * true_sensor_all + 23 e, true_counts[e] landmarks taken in order from true_ids_all / true_p_all (3 doubles each). nees[e], status[e] as eqf_batch_nees.
 * Returns 0, EQF_E_BAD_ARG or a HIP error. */
int eqvio_batch_compute_nees(eqvio_batch* b, int count, const int* slots, const double* true_sensor_all, const int* true_counts, const int* true_ids_all,
                             const double* true_p_all, double* nees, int* status);
/* The consistency record of `count` distinct slots in ONE launch (eqf_batch_consistency, include/eqf_batch.h): the argument list of eqvio_batch_compute_nees
 * with the records in place of nees. out[e].nees is eqvio_batch_compute_nees's value bit for bit; a refused entry's record is left untouched. Returns 0,
 * EQF_E_BAD_ARG or a HIP error. */
int eqvio_batch_consistency(eqvio_batch* b, int count, const int* slots, const double* true_sensor_all, const int* true_counts, const int* true_ids_all,
                            const double* true_p_all, eqf_batch_consistency_record* out, int* status);
/* augmentLandmarkStates(newIds, providedState) (VIOFilter.cpp:112-132) of `count` distinct slots in ONE launch (eqf_batch_augment). Entry e: slot slots[e],
 * new_counts[e] ids from new_ids_all, prov_counts[e] provided landmarks from prov_ids_all / prov_p_all. status[e] as eqf_batch_augment. Returns 0,
 * EQF_E_BAD_ARG or a HIP error. */
int eqvio_batch_augment_landmark_states(eqvio_batch* b, int count, const int* slots, const int* new_counts, const int* new_ids_all, const int* prov_counts,
                                        const int* prov_ids_all, const double* prov_p_all, int* status);
/* The reference's main_sim loop (src/main_sim.cpp:128-184, default mode) over the slots in lockstep: sims[k] is slot k's data server (NULL: the slot sits out).
 * Slot k starts from getInitialCondition() trimmed to the ids of its first image (initial-condition order: what the first augmentLandmarkStates leaves).
 * Per vision frame: every slot's IMU samples up to its next image, then ONE augment call (the image's ids, getTrueState(stamp, true)), ONE step and ONE NEES
 * call (getTrueState(time)) for every slot that has a frame. nees: max_frames x slots, row-major [frame][slot], NaN where a slot has no frame. Runs until
 * every sim has ended or max_frames frames have run; *frames_run = frames run. Returns 0, EQF_E_BAD_ARG, or -1 (a call failed: eqvio_batch_last_error). */
int eqvio_batch_run_sim(eqvio_batch* b, eqvio_sim* const* sims, int max_frames, double* nees, int* frames_run);
/* eqvio_batch_run_sim with the frame's NEES launch replaced by the consistency launch (eqf_batch_consistency): the same loop, the same nees array bit for
 * bit, and for every slot k with a sim the directory output_dir/run_<k>/ with the reference's consistency files of that run - nees.csv (NEES, DoF, PoseNEES,
 * AttitudeNEES), poseConsistency.csv, cameraConsistency.csv, biasConsistency.csv (the error components and the matching diagonal entries of Sigma) and
 * landmarkError.csv (one column per TRUE landmark, NaN where the slot does not hold it) - with the headers, column order and number formatting of the single
 * filter's `eqvio_sim --output` (VIOWriter). One row per frame the slot ran; a slot without a frame writes no row, and a file appears with its first row.
 * Only the records cross to the host. An output_dir that cannot be created gives -1 (eqvio_batch_last_error) before any frame runs; a null one EQF_E_BAD_ARG. */
int eqvio_batch_run_sim_recorded(eqvio_batch* b, eqvio_sim* const* sims, int max_frames, double* nees, int* frames_run, const char* output_dir);

/* The estimate records of `count` distinct slots in ONE launch (eqf_batch_estimates, include/eqf_batch.h: same records, same refusals, same codes; a refused
 * entry's record is left untouched) and, when times is not null, each listed slot's getTime(). A slot that has not initialised gives the state it was
 * created with (identity pose, the settings' camera offset, no landmark) and -1, as a single filter does. Returns 0, EQF_E_BAD_ARG (a null batch, slots, out
 * or status, count < 0) or a HIP error. */
int eqvio_batch_estimates(eqvio_batch* b, int count, const int* slots, eqf_batch_estimate_record* out, double* times, int* status);
/* getFeaturePredictions(cams[e], stamps[e]) (VIOFilter.cpp:247-252) of `count` distinct slots in ONE launch (eqf_batch_predictions, include/eqf_batch.h: same
 * records, a refused entry's record is left untouched). Per listed slot the (sample, dt) list is VIO_eqf::predictState's (VIO_eqf.cpp:139-151), from the slot's
 * own IMU buffer and current time: t0 = max(stamp_i, currentTime), t1 = min(stamp_{i+1}, stamps[e]) or stamps[e] for the last sample, dt = max(t1 - t0, 0).
 * out[e].y are the predicted pixels by id, out[e].out_cov the landmarks' output covariances at the current estimate (not propagated to the stamp, as the
 * reference's getOutputCovById). Like the reference, a slot whose settings have useFeaturePredictions == 0 gets N = 0 and every array zero, with sensor its
 * current estimate and status 0; it is not sent to the device, and if no entry is sent nothing is launched. A slot that has not initialised has no sample and
 * gives its current estimate (the state it was created with). status[e]: 0 or EQF_E_BAD_ARG (bad or repeated slot, bad camera). Nothing of any slot changes.
 * Returns 0, EQF_E_BAD_ARG (a null batch, slots, cams, stamps, out or status, count < 0), a HIP error or -1 (eqvio_batch_last_error). */
int eqvio_batch_feature_predictions(eqvio_batch* b, int count, const int* slots, const eqvio_camera* cams, const double* stamps, eqf_batch_prediction_record* out,
                                    int* status);
/* per slot: stateEstimate, viewEqFState (xi0, X, Sigma), getTime, isInitialised, and the forcing of a whole EqF state (teacher forcing) */
int eqvio_batch_state_estimate(eqvio_batch* b, int slot, double* sensor, int* ids, double* p, int cap); /* returns N or < 0 */
int eqvio_batch_get_eqf(eqvio_batch* b, int slot, double* xi0_sensor, double* X_sensor, int* ids, double* q0, double* Q, int cap);
int eqvio_batch_force_eqf(eqvio_batch* b, int slot, const double* xi0_sensor, const double* X_sensor, const int* ids, const double* q0, const double* Q, int N,
                          const double* sigma_colmajor);
int eqvio_batch_sigma_dim(const eqvio_batch* b, int slot);
int eqvio_batch_get_sigma(eqvio_batch* b, int slot, double* out_colmajor, int n);
double eqvio_batch_get_time(const eqvio_batch* b, int slot);
int eqvio_batch_is_initialised(const eqvio_batch* b, int slot);
/* Copies whole filters between slots without leaving the device (eqf_batch_copy_slots, include/eqf_batch.h: one launch, any mapping of sources to
 * destinations, same status codes and refusals): entry e makes slot dst[e] what slot src[e] was BEFORE the call - the EqF state (xi0, X, landmarks, Sigma) and
 * what the reference's VIOFilter keeps on the host: the IMU buffer, the current time and the initialised flag. The destination keeps its own settings and
 * its innovation totals; its last step's innovation reads 0, 0, 0. A refused entry changes nothing of its destination, host half included. For a sweep that
 * warms up once: run the first frames in one slot, copy it into the others, give them their settings. Returns 0, EQF_E_BAD_ARG (null arguments, count < 0)
 * or -1 (eqvio_batch_last_error). */
int eqvio_batch_copy_slots(eqvio_batch* b, int count, const int* src, const int* dst, int* status);
/* A whole filter between an eqvio_filter (include/eqvio_filter.h: the context path, one filter at low latency) and slots, without leaving the device: to
 * fork a live filter into what-if slots, or to hand the best of B tunings to the filter that runs in real time.
 * eqvio_batch_load_filter: every listed slot (distinct) becomes the filter - the EqF state by eqf_batch_load_ctx (include/eqf_batch.h: one launch for the whole
 * call, the same refusals and status codes) and what the reference's VIOFilter keeps on the host: the IMU buffer, the current time and the initialised flag
 * (the host half eqvio_batch_copy_slots moves). The destination keeps its own settings and innovation totals; a refused entry changes nothing, host half
 * included. The filter is not changed.
 * eqvio_batch_store_filter: the filter becomes the slot (eqf_batch_store_ctx, then the same host half); it keeps its own settings, the slot is unchanged.
 * Both return 0, an EQF_E_* code for refused arguments (nothing changed), or -1 (eqvio_batch_last_error). */
int eqvio_batch_load_filter(eqvio_batch* b, eqvio_filter* src, int count, const int* slots, int* status);
int eqvio_batch_store_filter(eqvio_batch* b, int slot, eqvio_filter* dst);
/* The innovation statistics of the slot's last step and their totals over the slot's updated steps (eqf_batch_last_innovation, _innovation_totals,
 * _reset_innovation_totals, include/eqf_batch.h: same meaning, same codes; the numbers are the device batch's, kept nowhere else). A slot that sits a step
 * out (stale stamp, ended sequence) adds nothing. For a score per slot of a replay: reset, eqvio_batch_run_prepared / _run_sim, read the totals. */
int eqvio_batch_last_innovation(const eqvio_batch* b, int slot, int* dof, double* nis, double* logdet);
int eqvio_batch_innovation_totals(const eqvio_batch* b, int slot, long* updates, long* dof, double* nis, double* logdet);
int eqvio_batch_reset_innovation_totals(eqvio_batch* b, int slot); /* slot < 0: every slot */
/* the device batch behind it */
eqf_batch* eqvio_batch_core(eqvio_batch* b);

#ifdef __cplusplus
}
#endif
#endif
