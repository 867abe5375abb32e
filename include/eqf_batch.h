/* eqf_batch.h — C-ABI of the filter batch: B independent EqF filters ("slots") of at most 64 landmarks each on one MI355X (gfx950),
 * advanced by one frame with ONE kernel launch (one workgroup per slot) and one host synchronisation per step.
 *
 * A slot is what one reference VIOFilter does in processVisionData (src/VIOFilter.cpp:194-241): the propagation - with fast Riccati (eqf_batch_step)
 * integrateRiccatiStateFast with the frame's mean IMU sample and the k observer steps, with the reference's default (eqf_batch_step_accurate) one
 * integrateRiccatiStateAccurate per sample between the observer steps, with the discrete state matrix (eqf_batch_step_discrete) one integrateRiccatiStateDiscrete
 * per sample in the same places -, removeOldLandmarks (settings.removeLostLandmarks), removeOutliers, addNewLandmarks (median or fixed depth),
 * performVisionUpdate and removeInvalidLandmarks. Its state is the one eqf_hip.h's context holds (xi0, X, Sigma; same flat layouts, eqvio_types.h).
 * The sensor-level work (the 46 doubles of xi0 / X, the terms of A and B, the observer steps' sensor part, the sensor lift) is done on the host, the
 * rest by the slot's workgroup. All three coordinate charts are available: Euclidean and InvDepth through the settings, Normal through a call of its own
 * (eqf_batch_set_slot_chart) - settings that name the Normal chart are still refused, as settings with fastRiccati == 0 are (EQF_E_UNSUPPORTED at creation). The
 * useDiscreteStateMatrix field of eqvio_settings is not read: the accurate and the discrete mode are calls of their own, not settings.
 * What remains refused of the Normal chart is the bridge to a context: eqf_batch_load_ctx / eqf_batch_store_ctx refuse a Normal-chart context.
 *
 * Return codes are eqf_hip.h's. Argument and settings checks come BEFORE the device is looked at: a call with bad arguments returns EQF_E_BAD_ARG /
 * EQF_E_UNSUPPORTED on a machine without a GPU as well; with valid arguments and no gfx950 device, eqf_batch_create returns EQF_E_NO_DEVICE.
 * A batch is bound to one device and one stream and must be used from one thread at a time.
 */
#ifndef EQF_BATCH_H
#define EQF_BATCH_H
#include "eqf_hip.h"
#include "eqvio_types.h"

#ifdef __cplusplus
extern "C" {
#endif

#define EQF_BATCH_MAX_LANDMARKS 64

typedef struct eqf_batch eqf_batch;

/* One slot's frame for eqf_batch_step. The measurement's ids are strictly ascending (the order of the reference's std::map). */
typedef struct eqf_batch_frame {
    int slot;
    eqvio_camera cam;
    const double* imu13_mean; /* the mean IMU sample of the Riccati step (VIOFilter.cpp:141-156) */
    double dt_total;
    int k;                    /* observer steps */
    const double* imu13_k;    /* k samples of 13 doubles */
    const double* dt_k;       /* their dts */
    int M;                    /* features */
    const int* ids;
    const double* y;          /* 2 M pixel coordinates */
} eqf_batch_frame;

/* Per-slot outcome of the last step (eqf_batch_last_result): which of removeOldLandmarks .. removeInvalidLandmarks happened */
enum {
    EQF_BATCH_REMOVED_OLD = 1,
    EQF_BATCH_REMOVED_OUTLIERS = 2,
    EQF_BATCH_ADDED = 4,
    EQF_BATCH_EMPTY = 8, /* the matched measurement was empty: no update (the reference's early return) */
    EQF_BATCH_UPDATED = 16,
    EQF_BATCH_REMOVED_INVALID = 32
};

/* slots >= 1, 1 <= max_landmarks <= 64; settings: fastRiccati must be 1 and the chart Euclidean or InvDepth (Normal: eqf_batch_set_slot_chart). Every slot starts with these settings and
 * keeps them until eqf_batch_set_slot_settings gives it its own: gains, thresholds, depth, lift choices and chart are per slot, so one step can run B
 * different tunings. Every slot starts with no landmark, Sigma = 0 and xi0 = X = identity (set them with eqf_batch_set_state / _set_sigma). */
int eqf_batch_create(eqf_batch** out, int device, int slots, int max_landmarks, const eqvio_settings* s);
void eqf_batch_destroy(eqf_batch* b);
int eqf_batch_slots(const eqf_batch* b);
int eqf_batch_max_landmarks(const eqf_batch* b);

/* The slot's own settings, from its next eqf_batch_step / _nees / _augment on; the other slots keep theirs. What a slot reads of them: the eight process
 * variances, the four IMU noises, measurementNoise, outlierThresholdAbs / Prob, featureRetention, initialPointVariance, initialSceneDepth, useMedianDepth,
 * useEquivariantOutput, useDiscreteInnovationLift, useDiscreteVelocityLift, removeLostLandmarks and coordinateChoice. The call launches nothing and does not
 * synchronise: the values travel in the slot's entry of the packet every step sends anyway. Refusals, checked in this order and before any device is
 * looked at; the slot and its settings are then untouched, bit for bit:
 *   EQF_E_BAD_ARG      null batch or settings, or a coordinateChoice outside the enum;
 *   EQF_E_UNSUPPORTED  fastRiccati == 0 or the Normal chart (as eqf_batch_create);
 *   EQF_E_BAD_ARG      bad slot index, or a chart other than the slot's while the slot holds landmarks: its Sigma is expressed in the old chart's
 *                      coordinates. On a slot without landmarks the chart may change (the sensor chart is the same for Euclidean and InvDepth).
 *                      eqf_batch_convert_chart changes the chart of a slot that holds landmarks, Sigma with it.
 * get returns what the slot runs with: the last accepted set, or eqf_batch_create's settings. */
int eqf_batch_set_slot_settings(eqf_batch* b, int slot, const eqvio_settings* s);
int eqf_batch_get_slot_settings(const eqf_batch* b, int slot, eqvio_settings* out);
/* What eqf_batch_create and eqf_batch_set_slot_settings make of these settings on their own: 0, EQF_E_BAD_ARG (null, or a coordinateChoice outside the enum)
 * or EQF_E_UNSUPPORTED (fastRiccati == 0 or the Normal chart). Looks at no device and no batch: a caller can refuse a whole list of settings up front. */
int eqf_batch_check_settings(const eqvio_settings* s);

/* The slot's coordinate chart on its own: EQVIO_COORD_EUCLIDEAN, EQVIO_COORD_INVDEPTH or EQVIO_COORD_NORMAL - the one way to the Normal chart, which the settings
 * calls above refuse. From the slot's next call on every step mode (eqf_batch_step, _step_accurate, _step_discrete), eqf_batch_nees / _consistency,
 * eqf_batch_predictions and the rest run the slot under that chart: its Sigma is then expressed in that chart's coordinates. A Normal slot's propagation is
 * the Euclidean one between two congruences with the chart's change of coordinates M (coordinateSuite/normal.cpp; k_batch_normal, k_batch_riccati_normal,
 * k_batch_discrete_normal), the rest of its frame the kernel every slot runs. One step may list slots of all three charts: one packet, one copy back and one
 * synchronisation as before, the Normal slots' propagation in launches of its own on the same stream; a slot gives the same bits whatever its neighbours' charts.
 * The call launches nothing and does not synchronise: the chart travels in the slot's packet entry like the other settings. Refusals, checked in this order
 * and before any device is looked at, the slot then untouched bit for bit:
 *   EQF_E_BAD_ARG      null batch or bad slot index; a chart outside the enum; a chart other than the slot's while the slot holds landmarks
 *                      (eqf_batch_set_slot_settings's rule). The slot's own chart is accepted on a slot with landmarks and does nothing.
 *                      eqf_batch_convert_chart changes the chart of a slot that holds landmarks, Sigma with it.
 * eqf_batch_get_slot_settings then reports the chart in coordinateChoice; a later accepted eqf_batch_set_slot_settings replaces it with its own (under the same
 * rule; Normal still refused there); eqf_batch_copy_slots and the bridge apply their chart rules to it as to the other two - a Normal slot with landmarks copies
 * into Normal slots only, and eqf_batch_store_ctx of it into a Euclidean or InvDepth context is the chart mismatch EQF_E_BAD_ARG. Moving a filter between a
 * Normal-chart CONTEXT and Normal slots is not built: eqf_batch_load_ctx / _store_ctx refuse such a context (EQF_E_UNSUPPORTED) as before.
 * get returns the slot's chart, or EQF_E_BAD_ARG (< 0) for a null batch or a bad slot. */
int eqf_batch_set_slot_chart(eqf_batch* b, int slot, int chart);
int eqf_batch_get_slot_chart(const eqf_batch* b, int slot);

/* The slot's xi0 / X / landmarks (eqf_set_state's layout: ids, q0 3 and Q 5 doubles per landmark). N <= max_landmarks. Sigma is NOT changed by set_state:
 * set it afterwards with eqf_batch_set_sigma (n = 21 + 3 N). get_state returns N or < 0. */
int eqf_batch_set_state(eqf_batch* b, int slot, const double* xi0_sensor, const double* X_sensor, const int* ids, const double* q0, const double* Q, int N);
int eqf_batch_get_state(eqf_batch* b, int slot, double* xi0_sensor, double* X_sensor, int* ids, double* q0, double* Q, int cap);
int eqf_batch_set_sigma(eqf_batch* b, int slot, const double* sigma_colmajor, int n);
int eqf_batch_get_sigma(eqf_batch* b, int slot, double* sigma_colmajor, int n);
int eqf_batch_num_landmarks(const eqf_batch* b, int slot);
/* stateGroupAction(X, xi0): the 23 sensor doubles, ids and landmark points (3 per landmark). Returns N or < 0. */
int eqf_batch_state_estimate(eqf_batch* b, int slot, double* sensor, int* ids, double* p, int cap);

/* stateGroupAction(X, xi0), sensor part: eqf_batch_state_estimate's 23 doubles, bit for bit, from the host's half of the slot alone - no device is looked at,
 * nothing is copied or synchronised. Returns 0, or EQF_E_BAD_ARG for a null batch, a bad slot or a null sensor. */
int eqf_batch_sensor_estimate(const eqf_batch* b, int slot, double* sensor);

/* Advances the `count` listed slots (distinct) by one frame each: one packet to the device, one launch, one copy back, one synchronisation.
 * A slot that is not listed is not touched, bit for bit. status[e] (count entries) is the result of entry e:
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index, repeated slot, ids not strictly ascending, bad camera: nothing of that slot was touched;
 *   EQF_E_CAPACITY     the frame would take the slot past max_landmarks (landmarks that stay + new ids), or its measurement has more than max_landmarks
 *                      features: refused before the launch, the slot is untouched;
 *   EQF_E_NOT_SPD      a pivot of the Cholesky factorisation of S = C Sigma C^T + R was <= 0;
 *   EQF_E_NONFINITE    Gamma was not finite. After these two the slot holds the frame's propagation and landmark bookkeeping (removeOldLandmarks,
 *                      removeOutliers, addNewLandmarks) without the vision update; the other slots are not affected.
 * The call itself returns 0 when the step ran (whatever the per-slot codes), EQF_E_BAD_ARG for null arguments, or a HIP error. */
int eqf_batch_step(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status);
/* eqf_batch_step with the reference's default propagation, fastRiccati == false (integrateUpToTime, src/VIOFilter.cpp:160-178): for sample i = 0 .. k-1, when
 * dt_i > 0, Sigma <- Phi Sigma Phi^T + Phi_B (Q / dt_i) Phi_B^T + dt_i P with [Phi Phi_B] the top n rows of exp(dt_i [[A, B], [0, 0]])
 * (integrateRiccatiStateAccurate, VIO_eqf.cpp:74-91), A and B at the X that samples 0 .. i-1 have produced, Q and P the slot's own gains; then the observer
 * step with sample i. A sample with dt_i == 0 skips its Riccati step and still runs its observer step. The rest of the frame is eqf_batch_step's, by the same
 * code. The frame struct, the screening, the status codes, the result flags, the innovation statistics and the totals are eqf_batch_step's; imu13_mean and
 * dt_total are not read and may be null / 0. In addition a dt_k that is negative or not finite gives EQF_E_BAD_ARG, the slot untouched bit for bit.
 * One packet to the device, one copy back and one synchronisation; two launches on the batch's stream between them (the per-sample propagation, then the frame's
 * remaining phases). The settings of a batch keep saying fastRiccati = 1: that field describes eqf_batch_step. Any slot may be advanced by either call in any
 * frame. */
int eqf_batch_step_accurate(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status);
/* eqf_batch_step_accurate with the discrete state matrix, fastRiccati == false and useDiscreteStateMatrix == true (integrateUpToTime, src/VIOFilter.cpp:165-170):
 * for sample i = 0 .. k-1, when dt_i > 0, Sigma <- A_d Sigma A_d^T + dt_i (B Q B^T + P) (integrateRiccatiStateDiscrete, VIO_eqf.cpp:93-103) with
 * A_d = stateMatrixADiscrete(X, xi0, imu_i, dt_i) (EqFMatrices.cpp:24-41: the central difference, h = cbrt(eps), of a0Discrete) and B = inputMatrixB, both at the X
 * that samples 0 .. i-1 have produced, Q and P the slot's own gains; then the observer step with sample i. A sample with dt_i == 0 skips its Riccati step and still
 * runs its observer step. A_d is formed on the device, its sensor part included (k_batch_discrete). Everything else is eqf_batch_step_accurate's: the frame struct,
 * the screening, the status codes, the result flags, the innovation statistics and the totals; imu13_mean and dt_total are not read and may be null / 0; a dt_k
 * that is negative or not finite gives EQF_E_BAD_ARG, the slot untouched bit for bit; one packet to the device, one copy back and one synchronisation, two
 * launches between them. Neither fastRiccati nor useDiscreteStateMatrix of the batch's settings says anything about this call: the mode is the call. Any slot may
 * be advanced by any of the three calls in any frame. eqf_batch_last_riccati then reports the samples with dt > 0, and 0 squarings. */
int eqf_batch_step_discrete(eqf_batch* b, int count, const eqf_batch_frame* frames, int* status);
/* Two counters of the slot's last eqf_batch_step_accurate / _discrete, written by its kernel into the result record: how many samples had dt > 0, and the largest
 * number of squarings an exponential of the step took (0: |dt [A B]|_inf <= 0.25 for every sample; always 0 after eqf_batch_step_discrete). After eqf_batch_step, or a copy into the slot
 * (eqf_batch_copy_slots, eqf_batch_load_ctx), both read 0. Null output pointers are skipped; a null batch or a bad slot gives EQF_E_BAD_ARG; no device is looked at. */
int eqf_batch_last_riccati(const eqf_batch* b, int slot, int* samples, int* max_squarings);
/* flags (EQF_BATCH_*) of the slot's last step, and the depth its new landmarks got */
int eqf_batch_last_result(const eqf_batch* b, int slot, int* flags, double* depth);

/* Innovation statistics of the slot's last step, taken from the factorisation the update does anyway (no extra launch, copy or synchronisation):
 *   dof     m, the rows of the matched measurement: two per feature left after removeOutliers, the features of new landmarks included;
 *   nis     the normalised innovation squared yTilde^T S^-1 yTilde;
 *   logdet  log det S,
 * with S = C Sigma C^T + R the innovation covariance of performVisionUpdate, formed with the slot's own measurementNoise and useEquivariantOutput. The
 * innovation log-likelihood is left to the caller: -1/2 (nis + logdet + dof ln 2 pi). What the last step leaves:
 *   EQF_BATCH_UPDATED                    m, the values;
 *   EQF_BATCH_EMPTY                      0, 0, 0;
 *   EQF_E_NOT_SPD / EQF_E_NONFINITE      m, NaN, NaN (no update was applied);
 *   refused before the launch (EQF_E_BAD_ARG, EQF_E_CAPACITY) or not listed: unchanged; a slot that never stepped has 0, 0, 0.
 * A slot gives the same bits whichever step it is part of: the sums have a fixed order.
 * The totals are the sums, formed on the host in step order, over the slot's steps that carried EQF_BATCH_UPDATED (failed and empty steps add nothing), and
 * the number of those steps. Only eqf_batch_reset_innovation_totals (slot < 0: every slot) clears them: eqf_batch_set_state, _set_sigma and
 * _set_slot_settings leave them, so a teacher-forced loop keeps its totals. Null output pointers are skipped. A null batch or a bad slot gives
 * EQF_E_BAD_ARG; no device is looked at. */
int eqf_batch_last_innovation(const eqf_batch* b, int slot, int* dof, double* nis, double* logdet);
int eqf_batch_innovation_totals(const eqf_batch* b, int slot, long* updates, long* dof, double* nis, double* logdet);
int eqf_batch_reset_innovation_totals(eqf_batch* b, int slot);

/* One slot's true state for eqf_batch_nees: the 23 sensor doubles (eqvio_types.h layout) and n_true landmarks, ids in any order, camera-frame points. */
typedef struct eqf_batch_truth {
    int slot;
    const double* sensor;
    int n_true;
    const int* ids;
    const double* p; /* 3 n_true */
} eqf_batch_truth;

/* computeNEES (VIO_eqf.cpp:153-170) of the `count` listed slots (distinct): one packet to the device, one launch (one workgroup per entry), one copy back,
 * one synchronisation. nees[e] is entry e's NEES; status[e]:
 *   0                  done: a Cholesky factorisation of [Sigma ; eps^T], or, when a pivot was <= 0, partial-pivot elimination on [Sigma | eps]
 *                      (eqf_batch_nees_lu_fallbacks counts those), as eqf_compute_nees;
 *   EQF_E_BAD_ARG      bad slot index, repeated slot, null pointers, or a filter landmark id missing from the truth (the reference asserts there).
 * The call is read-only: no slot's state, Sigma or landmark planes change. Returns 0 when the launch ran (whatever the per-entry codes), EQF_E_BAD_ARG for
 * null arguments or count < 0, or a HIP error. */
int eqf_batch_nees(eqf_batch* b, int count, const eqf_batch_truth* truths, double* nees, int* status);
/* how many eqf_batch_nees entries of the slot took the partial-pivot fallback */
int eqf_batch_nees_lu_fallbacks(const eqf_batch* b, int slot, long* count);

/* The blocks of the sensor state a consistency record reports, and their rows of eps / Sigma (nees_sensor_error's order: gyroscope and accelerometer bias,
 * attitude, position, velocity, camera attitude and position): 0..5, 6..8, 9..11, 6..11, 12..14, 15..20, 0..20. */
enum { EQF_BLOCK_BIAS, EQF_BLOCK_ATTITUDE, EQF_BLOCK_POSITION, EQF_BLOCK_POSE, EQF_BLOCK_VELOCITY, EQF_BLOCK_CAMERA, EQF_BLOCK_SENSOR, EQF_BATCH_NBLOCKS };

/* One slot's consistency record: what the reference's Monte-Carlo study writes per frame (VIOWriter::writeConsistency, writeLandmarkError) beside the full NEES.
 * n = 21 + 3 N. Entries of the fixed-size arrays beyond n or N read 0. */
typedef struct eqf_batch_consistency_record {
    int N, lu;                       /* landmarks of the slot; 1: the full NEES took the partial-pivot fallback */
    double nees;                     /* as eqf_batch_nees: eps^T Sigma^-1 eps / n */
    double block[EQF_BATCH_NBLOCKS]; /* x^T M^-1 x of the block, NOT divided by its dof (nees.csv's PoseNEES / AttitudeNEES) */
    double eps[21 + 3 * EQF_BATCH_MAX_LANDMARKS];        /* the eps computeNEES forms */
    double sigma_diag[21 + 3 * EQF_BATCH_MAX_LANDMARKS]; /* the diagonal of Sigma */
    int ids[EQF_BATCH_MAX_LANDMARKS];                    /* state order */
    double lm_quad[EQF_BATCH_MAX_LANDMARKS];             /* eps_i^T Sigma_ii^-1 eps_i, 3 x 3 marginal of landmark i */
    double lm_err[EQF_BATCH_MAX_LANDMARKS];              /* |p_hat_i - p_true_i|, camera frame (landmarkError.csv) */
} eqf_batch_consistency_record;

/* The consistency record of the `count` listed slots (distinct): one packet to the device, one launch (one workgroup per accepted entry), one copy back, one
 * synchronisation; nothing but the records crosses to the host. Arguments, refusals and codes are eqf_batch_nees's (status[e] 0 or EQF_E_BAD_ARG; the call
 * returns EQF_E_BAD_ARG for null arguments or count < 0), checked before any device is looked at; a refused entry's record is left untouched. out[e].nees and
 * out[e].lu are, bit for bit, what eqf_batch_nees gives for the same entry (the same factorisation, the same fallback), and the fallback counts in
 * eqf_batch_nees_lu_fallbacks in the same way. The block forms and the landmarks' 3 x 3 forms are x^T M^-1 x by Gaussian elimination with partial pivoting on
 * [M | x] (the reference's .inverse() route); a zero pivot gives a non-finite value, reported as it is. The landmark's point estimate is
 * eqf_batch_state_estimate's. The call is read-only like eqf_batch_nees: no slot's state, Sigma, landmark planes, settings, innovation totals or last result
 * change. */
int eqf_batch_consistency(eqf_batch* b, int count, const eqf_batch_truth* truths, eqf_batch_consistency_record* out, int* status);

/* One slot's state estimate: what stateEstimate() and viewEqFState() hand back of a filter for its output files, in one fixed-size record. Entries of the
 * fixed-size arrays beyond N read 0. The sensor layout is eqvio_types.h's (bias, pose quaternion and position, velocity, camera offset). */
typedef struct eqf_batch_estimate_record {
    int N, reserved;                                /* landmarks of the slot; 0 */
    double sensor[23];                              /* stateGroupAction(X, xi0), sensor part: eqf_batch_state_estimate's 23 doubles */
    double sigma_sensor[21 * 21];                   /* Sigma[0:21, 0:21], column-major */
    int ids[EQF_BATCH_MAX_LANDMARKS];               /* state order */
    double p[3 * EQF_BATCH_MAX_LANDMARKS];          /* camera-frame points, Q^-1 q0 (eqf_batch_state_estimate's p) */
    double p_world[3 * EQF_BATCH_MAX_LANDMARKS];    /* pose * cameraOffset * p: the points of points.csv */
} eqf_batch_estimate_record;

/* The state estimates of the `count` listed slots (distinct): one packet to the device, one launch (k_batch_estimate, one workgroup per accepted entry), one
 * copy back, one synchronisation, whatever count is; nothing but the records crosses to the host. The host supplies what it holds of a slot (its current
 * buffers, N, the ids, the sensor estimate - by the function eqf_batch_state_estimate uses, so N, ids and sensor are that call's bit for bit - and the product
 * pose * cameraOffset); the slot's workgroup reads its landmark planes and Sigma and writes p, p_world and sigma_sensor. sigma_sensor is the raw block of
 * Sigma, as eqf_batch_get_sigma returns it, bit for bit; p and p_world are formed on the device and agree with eqf_batch_state_estimate's p to rounding.
 * The call is read-only: no slot's state, Sigma, landmark planes, settings, innovation totals, last result or LU-fallback count change. A slot's record has
 * the same bytes whichever call it is part of: alone, among others in any order, in a batch of any size (nothing is summed). status[e]:
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index or repeated slot: out[e] is left untouched, byte for byte; the other entries are still done.
 * Returns 0 when the launch ran (whatever the per-entry codes) or count == 0, EQF_E_BAD_ARG for a null batch, slots, out or status or count < 0 (checked
 * before any device is looked at), or a HIP error. */
int eqf_batch_estimates(eqf_batch* b, int count, const int* slots, eqf_batch_estimate_record* out, int* status);

/* One slot's prediction request for eqf_batch_predictions: the camera, and the (sample, dt) list VIO_eqf::predictState would integrate. */
typedef struct eqf_batch_prediction_entry {
    int slot;
    eqvio_camera cam;
    int k;                 /* steps of predictState, >= 0 */
    const double* imu13_k; /* k samples of 13 doubles (eqf_batch_frame's layout); may be null when k == 0 */
    const double* dt_k;    /* their dts, each >= 0 */
} eqf_batch_prediction_entry;

/* One slot's feature predictions. Entries of the fixed-size arrays beyond N read 0. */
typedef struct eqf_batch_prediction_record {
    int N, reserved;                              /* landmarks of the slot; 0 */
    double sensor[23];                            /* sensor part of the predicted state (eqvio_types.h layout) */
    int ids[EQF_BATCH_MAX_LANDMARKS];             /* state order */
    double p[3 * EQF_BATCH_MAX_LANDMARKS];        /* predicted camera-frame points */
    double y[2 * EQF_BATCH_MAX_LANDMARKS];        /* their pixels: cam.projectPoint(p) */
    double out_cov[4 * EQF_BATCH_MAX_LANDMARKS];  /* getOutputCovById at the CURRENT estimate, row-major 2 x 2 */
} eqf_batch_prediction_record;

/* What VIOFilter::getFeaturePredictions (VIOFilter.cpp:247-252) and VIO_eqf::getOutputCovById (VIO_eqf.cpp:196-211) give, for the `count` listed slots
 * (distinct): one packet to the device, one launch (k_batch_predict, one workgroup per accepted entry, a lane per landmark), one copy back, one
 * synchronisation, whatever count is; nothing but the records crosses to the host.
 * The predicted state is stateGroupAction(X, xi0) taken through integrateSystemFunction(state, imu_j, dt_j) for j = 0 .. k-1 (VIO_eqf::predictState's loop
 * with the dts given). The host does the chain's sensor part - sensor is its result - and folds the steps' cameraPoseChangeInv into one pose T; the slot's
 * workgroup forms p_i = T Q_i^-1 q0_i from its current landmark planes and y_i = cam.projectPoint(p_i). k == 0 gives the current estimate and its pixels:
 * the yHat of removeOutliers, with p equal to eqf_batch_state_estimate's to rounding. A landmark whose predicted depth is <= 0 gets whatever the camera
 * model's projection gives for it (non-finite or mirrored pixels), as in the single filter: it is not flagged.
 * out_cov[4 i ..] is C0_i Sigma_ii C0_i^T with C0_i = outputMatrixCi at the slot's current xi0, X, Sigma and chart for entries[e].cam - eqf_output_cov_all's
 * quantity. It does not depend on k, imu13_k or dt_k: like the reference's getOutputCovById it is not propagated to the stamp.
 * The call is read-only: no slot's state, Sigma, landmark planes, settings, innovation totals, last innovation, last result or LU-fallback count change. A
 * slot's record has the same bytes whichever call it is part of: alone, among others in any order, in a batch of any size (nothing is summed). status[e]:
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index, repeated slot, bad camera, k < 0, k > 0 with a null imu13_k or dt_k, or a dt that is negative or not finite: out[e]
 *                      is left untouched, byte for byte; the other entries are still done.
 * Returns 0 when the launch ran (whatever the per-entry codes) or count == 0, EQF_E_BAD_ARG for a null batch, for null entries, out or status with
 * count > 0, or for count < 0 (checked before any device is looked at), or a HIP error. */
int eqf_batch_predictions(eqf_batch* b, int count, const eqf_batch_prediction_entry* entries, eqf_batch_prediction_record* out, int* status);

/* One slot's augmentLandmarkStates for eqf_batch_augment: the ids the slot keeps and adds (n_new), and the provided state's landmarks (n_prov ids and
 * camera-frame points) the new ones are taken from. */
typedef struct eqf_batch_augment_entry {
    int slot;
    int n_new;
    const int* new_ids;
    int n_prov;
    const int* prov_ids;
    const double* prov_p; /* 3 n_prov */
} eqf_batch_augment_entry;

/* VIOFilter::augmentLandmarkStates(newIds, providedState) (VIOFilter.cpp:112-132) of the `count` listed slots (distinct), one launch (one workgroup per entry
 * that changes its slot): landmarks whose id is not in new_ids leave the state; ids of new_ids not in the state are appended in new_ids order, q0 = the
 * provided point, Q = identity, with zero cross terms and initialPointVariance I in Sigma. status[e]:
 *   0                  done (an entry that neither removes nor adds leaves its slot as it is, bit for bit);
 *   EQF_E_BAD_ARG      bad or repeated slot, null pointers, or a new id without a provided point: the slot is untouched;
 *   EQF_E_CAPACITY     the result would hold more than max_landmarks: the slot is untouched.
 * Returns 0, EQF_E_BAD_ARG for null arguments or count < 0, or a HIP error. */
int eqf_batch_augment(eqf_batch* b, int count, const eqf_batch_augment_entry* entries, int* status);

/* Copies whole filters between slots on the device: entry e makes slot dst[e] hold the EqF state slot src[e] held BEFORE the call - xi0, X, the landmark
 * ids, the landmarks (q0 and its chart constants, Q) and Sigma (n x n, n = 21 + 3 N), bit for bit. One launch for the whole call and one synchronisation;
 * nothing crosses to the host. Every copy reads its source's current buffers and writes its destination's other ones, so the entries of one call may form
 * any mapping: a slot may be the source of many entries, and the destination of one entry while the source of another (a swap, a cycle). To fork a run, to
 * warm up once and branch into B tunings, to resample by likelihood, to keep a checkpoint slot.
 * The destination keeps its own settings (eqf_batch_set_slot_settings), its innovation totals and its eqf_batch_nees_lu_fallbacks count. Its last step's
 * outcome was another state's: eqf_batch_last_result gives flags 0 and depth 0, eqf_batch_last_innovation 0, 0, 0, as on a slot that never stepped.
 * src[e] == dst[e] is accepted and does nothing, but it names its slot as a destination like any entry: a later entry into that slot is refused as a
 * repeated destination, and so is the entry onto itself when an earlier entry copied into the slot. status[e] (count entries):
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index; a destination that an earlier entry of the call names already; or a source that holds landmarks while the
 *                      destination's coordinateChoice is not the source's: Sigma is expressed in the chart's coordinates (the rule of
 *                      eqf_batch_set_slot_settings; a source without landmarks copies into either chart). eqf_batch_convert_chart on the
 *                      destination afterwards, or on the source before, takes a filter across charts.
 * Refusals are decided before any device work and leave the refused destination untouched, bit for bit; the other entries are still done.
 * Returns 0 when the launch ran (whatever the per-entry codes), EQF_E_BAD_ARG for a null batch, src, dst or status or count < 0 (no device is looked at),
 * or a HIP error. */
int eqf_batch_copy_slots(eqf_batch* b, int count, const int* src, const int* dst, int* status);

/* Changes the chart of slots that hold landmarks, on the device: entry e re-expresses slot slots[e] in chart charts[e] (EQVIO_COORD_*). The three charts differ
 * by a constant, block-diagonal change of coordinates that depends on xi0 alone (coordinateDifferential_invdepth_euclid / _normal_euclid, VIOState.cpp:355-401):
 * with M_euclid = I, M_invdepth = blockdiag(I_21, conv_euc2ind(q0_i)) and M_normal the Normal chart's M (sensor block from xi0's velocity and Ad(T0^-1), landmark
 * blocks normal_M(q0_i)), Sigma <- T Sigma T^T with T = M_to M_from^-1. It is the same filter, described differently:
 *   - xi0, X, the ids, q0 and Q do not change, bit for bit; the landmark planes the new chart reads are rebuilt from q0 by the function every landmark-creating
 *     kernel calls;
 *   - the slot's coordinateChoice becomes the new chart (eqf_batch_get_slot_chart, _get_slot_settings); every other setting, the innovation totals, the last
 *     result, the last innovation, the last Riccati counters and the eqf_batch_nees_lu_fallbacks count are kept.
 * One launch of k_batch_rechart for the whole call (one workgroup per entry that changes something on the device) and one synchronisation; nothing of Sigma
 * crosses to the host. The kernel reads the slot's current buffers and writes its other ones, which then become current. The lower half of Sigma' is computed in
 * a fixed order - (T_i Sigma_ij), then (. T_j^T) - and mirrored, so Sigma' is symmetric bit for bit; when neither chart is Normal the 21 x 21 sensor block is
 * copied bit for bit. A slot's result has the same bytes whichever call and batch it is part of.
 * Launching nothing: an entry whose chart is the slot's already does nothing, bit for bit; an entry on a slot without landmarks, neither chart Normal, is
 * eqf_batch_set_slot_chart's relabelling (a slot without landmarks still goes to the device when one chart is Normal: the sensor block of Sigma changes).
 * The process noise P is diagonal in each chart's own coordinates, so two filters that differ by a conversion stop being the same filter with their next
 * propagation. With useEquivariantOutput = 0 the innovation covariance S = C Sigma C^T + R is unchanged by a conversion to rounding; the Normal chart's
 * equivariant output is not the transported Euclidean one.
 * status[e], decided before any device is looked at - a refused slot is untouched bit for bit, the other entries are still done:
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index, a slot an earlier entry of the call names, or a chart outside the enum.
 * Returns 0 when it ran (whatever the per-entry codes) or count == 0, EQF_E_BAD_ARG for a null batch, slots, charts or status or count < 0 (no device is looked
 * at), or a HIP error. */
int eqf_batch_convert_chart(eqf_batch* b, int count, const int* slots, const int* charts, int* status);

/* The bridge between a context (eqf_hip.h: one filter at low latency) and the slots, on the device: to fork a running filter into B what-if slots, to warm a
 * sweep up on the fast path, to put the best of B tunings back into the filter that runs in real time.
 *
 * eqf_batch_load_ctx: every listed slot (distinct) comes to hold what the context holds - xi0, X, the landmark ids in state order, per landmark q0, Qq and Qa,
 * and Sigma (n x n, n = 21 + 3 N): eqf_batch_get_state / _get_sigma of the slot then equal eqf_get_state / eqf_get_sigma of the context, bit for bit, and the
 * slot is the one eqf_batch_set_state + _set_sigma with those values would have made, bit for bit in every later frame (the landmarks' chart constants are
 * formed from q0 by the function those calls use). One launch for the whole call, whatever count is, and one synchronisation; nothing of Sigma or the landmark
 * planes crosses to the host (the 46 sensor doubles and the ids live on the host on both sides and are copied there). The kernel reads the context's current
 * buffers with their own plane stride and leading dimension and writes each destination's other buffers, which then become current: nothing the slot held
 * before shows. The context is entered as by eqf_get_state (an update taken from the early doorbell is settled, held landmarks and a pending reshape are
 * applied, the observer's stream is joined) and is otherwise not changed in any way its API can show.
 * The destination keeps its own settings, its innovation totals and its eqf_batch_nees_lu_fallbacks count; its last result and last innovation read as on a
 * slot that never stepped (eqf_batch_copy_slots's rule). Refusals are decided before any device work. Of the whole call - no slot is touched, status is not
 * written:
 *   EQF_E_BAD_ARG      null b, src, slots or status, or count < 0 (also on a machine without a GPU); a context on another device than the batch;
 *   EQF_E_UNSUPPORTED  a context with the Normal chart (its sensor block of Sigma is in other coordinates) or the float Sigma store (EQF_OPT_SIGMA_FP32 = 2);
 *   EQF_E_CAPACITY     the context holds more landmarks than eqf_batch_max_landmarks(b).
 * Per entry, status[e] - the other entries are still done, a refused slot is untouched bit for bit:
 *   0                  done;
 *   EQF_E_BAD_ARG      bad slot index; a slot an earlier accepted entry of the call names; or a slot whose coordinateChoice is not the context's chart while
 *                      the context holds landmarks (eqf_batch_set_slot_settings's rule; a context without landmarks loads into either chart).
 * Returns 0 when it ran (whatever the per-entry codes) or count == 0, one of the codes above, or a HIP error.
 *
 * eqf_batch_store_ctx: the context comes to hold what the slot holds, exactly as after eqf_set_state + eqf_set_sigma with the slot's values - the estimate
 * cache, a staged measurement, held landmarks and the id lookups are dropped, the landmark generation moves on, the capacity grows when the slot holds more
 * landmarks than the context has room for - with one launch and one synchronisation and neither Sigma nor the planes over the bus (a context with
 * EQF_OPT_SIGMA_FP32 = 1 rounds Sigma behind it, as eqf_set_sigma does). The slot is unchanged. Refusals, the context untouched:
 *   EQF_E_BAD_ARG      null b or dst, a bad slot, a context on another device; a slot with landmarks whose coordinateChoice is not the context's chart;
 *   EQF_E_UNSUPPORTED  a Normal-chart or float-store context.
 * A slot of another chart is stored after eqf_batch_convert_chart has taken it to the context's chart.
 * Returns 0, one of these codes, EQF_E_CAPACITY when the context could not grow, or a HIP error. */
int eqf_batch_load_ctx(eqf_batch* b, eqf_ctx* src, int count, const int* slots, int* status);
int eqf_batch_store_ctx(eqf_batch* b, int slot, eqf_ctx* dst);
/* the hipStream_t the batch launches on, as void* */
void* eqf_batch_stream(eqf_batch* b);
int eqf_batch_synchronize(eqf_batch* b);

#ifdef __cplusplus
}
#endif
#endif
