// eqvio_opt: the reference's dataset main (src/main_opt.cpp:178-269) on the MI355X EqF path, fed by precomputed feature
// tracks instead of images (no OpenCV / GIFT here): IMU -> processIMUData, tracks -> processVisionData, outputs through
// VIOWriter. The filter starts uninitialised and sets its attitude from the first IMU sample (VIOFilter.cpp:65-78).
// --batch B [--sweep NAME=v0,...] replays the dataset in the B slots of one filter batch (VIOFilterBatch.hpp), slot k with the k-th value, and scores every
// slot by its innovation statistics (include/eqf_batch.h): a tuning sweep on a dataset without landmark truth. With --warmup F the first F frames run once, in
// slot 0 under the command line's settings, and slot 0 is then copied into the other slots on the device (eqf_batch_copy_slots): every tuning starts from the
// same converged filter, and the scores count the frames after the warm-up only. With --warmupOnFilter the F frames run on one VIOFilter instead (the context
// path, the fastest way this repository runs a single filter), which is then loaded into all B slots on the device (eqf_batch_load_ctx).
// --batch B --warmup F --rechart c0[,c1,...] converts slot k to chart ck at the branch (eqf_batch_convert_chart): one warm-up, B charts from the same belief.
// --batch B --record DIR writes every slot's trajectory (the four state files of --output) to DIR/run_<k>/, and --batch B --groundtruth FILE scores every slot's
// trajectory against ground truth: both from ONE estimates call per vision measurement over the live slots (eqf_batch_estimates).
// --batch B --predictions scores every slot by how far a frame's measured features lie from where the slot predicted them (getFeaturePredictions at the
// measurement's stamp, before the step): ONE predictions call per vision measurement over the live slots (eqf_batch_predictions).
// --branchAt F --branchCharts c0[,c1,...] (no --batch): F vision frames on one filter, which is then copied on the device into one fresh filter per chart
// (eqf_copy_ctx), each copy converted to its chart (eqf_convert_chart); every branch runs the remaining frames and prints its scores, labelled with its chart.
#include "DatasetReplay.hpp"
#include "VIOFilterBatch.hpp"
#include "VIOWriter.hpp"
#include "cli.hpp"
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <iostream>

using namespace eqvio_amd;

static void check_rc(int rc, const char* what) {
    if (rc != 0)
        throw std::runtime_error(std::string(what) + ": " + eqf_error_string(rc));
}

static void usage() {
    std::puts("usage: eqvio_opt --imu FILE --features FILE [--format asl|uzhfpv] [--groundtruth FILE] [--dumpMeasurements] [--dumpStates FILE] [--printCamera]\n"
              "                 [--cameraFile sensor.yaml | camchain.yaml]   (intrinsics, distortion and camera offset from the dataset's own file, main_opt.cpp:114-147)\n"
              "                 [--camera fx fy cx cy width height] [--distortion radtan k1 k2 p1 p2 k3 | --distortion equidistant k1 k2 k3 k4]\n"
              "                 [--cameraOffset qw qx qy qz x y z] [--cameraLag S] [--start S] [--stop S] [--output DIR] [--sigmaFP32] [--quiet]\n"
              "                 [--batch B [--sweep NAME=v0,v1,... [--warmup F [--warmupOnFilter]]] [--record DIR] [--predictions]\n"
              "                 [--nis] [--branchAt F --branchCharts euclidean|invdepth|normal[,...]]\n"
              "                            [--batchRiccati fast|accurate|discrete[,...]]\n"
              "                            [--batchChart euclidean|invdepth|normal[,...]]\n"
              "                            [--warmup F --rechart euclidean|invdepth|normal[,...]]]\n"
              "                 [--<eqf setting> VALUE ...]   (names of VIOFilter::Settings, e.g. --fastRiccati 1 --coordinateChoice InvDepth)\n"
              "  --batch B   replays the dataset in B slots of one filter batch (include/eqvio_batch.h): per measurement every slot's IMU samples, then ONE\n"
              "              vision step over all slots. Prints one line per slot: vision updates, mean normalised innovation squared per degree of freedom\n"
              "              (sum NIS / sum dof: about 1 for a consistent filter) and the total innovation log-likelihood. Needs --fastRiccati 1 and at most 64\n"
              "              features per frame; --output, --dumpStates and --sigmaFP32 are refused. With --groundtruth FILE one more line per slot: the position\n"
              "              RMSE of the slot's trajectory against the ground-truth poses nearest in time, after aligning the first poses.\n"
              "  --nis   a single-filter run (no --batch): switches the device context's innovation statistics on (EQF_OPT_INNOVATION_STATS) and prints, after the\n"
              "              run, the frames updated, the mean NIS per degree of freedom and the total innovation log-likelihood, in the wording of --batch's slot lines\n"
              "  --branchAt F --branchCharts C[,C...]   a single-filter run (no --batch): the first F vision frames run on one filter under the settings' chart; that\n"
              "              filter is then copied on the device into one fresh filter per chart C_k, each copy is converted to its chart (Sigma goes into the new\n"
              "              chart's coordinates; the state does not change), and every branch runs the remaining frames. Prints per branch, labelled with its chart,\n"
              "              the final state and, with --nis / --groundtruth, the single filter's scores over the frames after the branch. Any landmark count the\n"
              "              single filter runs. --output, --dumpStates and --sigmaFP32 are refused beside it.\n"
              "  --record DIR   with --batch B: slot k's IMUState.csv, camera.csv, bias.csv and points.csv (the formats of --output) go to DIR/run_<k>/, one row per\n"
              "              vision measurement per live slot, from one estimates call over the live slots per measurement. With --warmup F slots 1 .. B-1 start\n"
              "              their files at the branch.\n"
              "  --predictions   with --batch B: switches useFeaturePredictions on and, per vision measurement, asks every live slot where it expects its\n"
              "              landmarks at the measurement's stamp (one predictions call over the live slots, after the IMU samples, before the step). Prints one\n"
              "              more line per slot: the RMSE in pixels between predicted and measured features over the ids present in both - a score of the\n"
              "              propagation side of a tuning that needs no true state. With --warmup F the frames after the warm-up count.\n"
              "  --sweep NAME=v0,...,v(B-1)   with --batch B: slot k runs with the filter setting NAME (a field of eqvio_settings) at value vk. Needs exactly B values.\n"
              "  --warmup F   with --batch B --sweep: the first F vision frames run in slot 0 alone, with the command line's settings; slot 0 is then copied into\n"
              "              slots 1 .. B-1 on the device, the sweep's values go to all B slots, and the scores count the frames after the warm-up only.\n"
              "              With F > 0 a sweep of coordinateChoice (Sigma is in the chart's coordinates) or of an initial variance of the sensor state (used only\n"
              "              when a filter starts) is refused.\n"
              "  --warmupOnFilter   with --warmup F (F > 0): the F warm-up frames run on ONE single filter (the low-latency context path) with the command line's\n"
              "              settings instead of in slot 0; the filter is then loaded into all B slots on the device in one call, the sweep's values are applied and\n"
              "              scoring starts. With --record DIR every slot starts its files at the branch.\n"
              "  --batchRiccati M[,M...]   with --batch B: the slots' propagation, M = fast (one fast Riccati step per frame), accurate (the reference's default,\n"
              "              fastRiccati: false: one accurate Riccati step per IMU sample) or discrete (accurate with the discrete state matrix,\n"
              "              useDiscreteStateMatrix: true); one value for every slot, or B values, one per slot. With this flag\n"
              "              --fastRiccati 1 need not be given: the tool hands the batch that setting itself. Each slot's lines name its mode.\n"
              "  --batchChart C[,C...]   with --batch B: the slots' coordinate chart, C = euclidean, invdepth or normal (the reference's third chart, which\n"
              "              --coordinateChoice and --sweep coordinateChoice=... do not take with --batch); one value for every slot, or B values, one per slot.\n"
              "              Combines with --batchRiccati and --sweep, not with --warmup F > 0 (the chart cannot change under a filter that holds landmarks).\n"
              "              Each slot's lines name its chart.\n"
              "  --rechart C[,C...]   with --batch B --warmup F (F > 0; --sweep is not needed, and may stand beside it): the warm-up runs under the settings'\n"
              "              chart and is copied or loaded into the B slots as above; slot k is then converted to chart C_k on the device (Sigma goes into the new\n"
              "              chart's coordinates; the state does not change) and the frames after F are scored. One value for every slot, or B values, one per\n"
              "              slot. Not with --batchChart or --sweep coordinateChoice=.... Each slot's lines name its chart.");
}

// --batch B: the loop of main() for B slots of one filter batch over the same measurements; slot k with the sweep's k-th value
static int runBatch(TrackReplayServer& dataServer, const VIOFilter::Settings& fs, int B, const Sweep& sweep, int warmup, double startTime, double stopTime,
                    const std::string& recordDir, const std::vector<StampedPose>* groundtruth, bool predictions, bool warmupOnFilter, const std::vector<int>& riccati,
                    const std::vector<int>& charts, const std::vector<int>& rechart) {
    const bool swept = !sweep.name.empty();
    const eqvio_settings es = batchSettings(fs);
    eqf_batch* core = nullptr;
    if (const int rc = eqf_batch_create(&core, fs.device, B, EQF_BATCH_MAX_LANDMARKS, &es)) {
        std::fprintf(stderr, "eqvio_opt: eqf_batch_create: %s\n", eqf_error_string(rc));
        return 1;
    }
    VIOFilterBatch filters(core); // every slot as VIOFilter(fs): it initialises itself from its first IMU sample
    for (int k = 0; k < B && !riccati.empty(); ++k) // kept through the warm-up's copies, like the settings
        check_rc(filters.setRiccatiMode(k, batchCliRiccati(riccati[k])), "--batchRiccati"), check_rc(filters.setStateMatrix(k, batchCliStateMatrix(riccati[k])), "--batchRiccati");
    auto label = [&](int k) {
        return (swept ? " " + sweep.name + "=" + sweep.values[k] : std::string()) + (riccati.empty() ? std::string() : std::string(" riccati ") + batchRiccatiName(riccati[k])) +
               (charts.empty() ? std::string() : std::string(" chart ") + batchChartName(charts[k])) +
               (rechart.empty() ? std::string() : std::string(" chart ") + batchChartName(rechart[k]));
    };
    // --warmupOnFilter: the warm-up's frames run here, on the context path, and no slot runs before the branch
    std::unique_ptr<VIOFilter> warm;
    if (warmupOnFilter) {
        loopTimer.initialise({"correction", "features", "preprocessing", "propagation", "total", "total vision update", "write output"});
        warm = std::make_unique<VIOFilter>(fs);
    }
    // --record / --groundtruth: the live slots' estimates after every vision measurement, one call for all of them
    const bool wantEstimates = !recordDir.empty() || groundtruth;
    std::vector<std::unique_ptr<VIOWriter>> writers(B);
    for (int k = 0; k < B && !recordDir.empty(); ++k)
        writers[k] = makeRunWriter(recordDir, k); // before any frame runs
    std::vector<eqf_batch_estimate_record> records(B);
    std::vector<std::vector<StampedPose>> trajectories(B);
    // --predictions: per slot the sum of |y_pred - y_meas|^2 over the ids in both, and their number
    std::vector<eqf_batch_prediction_record> predicted(predictions ? B : 0);
    std::vector<eqvio_camera> predCams(B);
    std::vector<double> predStamps(B), predSq(B, 0.0);
    std::vector<long> predCount(B, 0);
    auto applySweep = [&] {
        for (int k = 0; k < B && swept; ++k) {
            eqvio_settings ek = es;
            std::string why;
            setSettingsField(ek, sweep.name, sweep.values[k], why);
            if (const int rc = filters.setSlotSettings(k, ek))
                throw std::runtime_error("--sweep " + sweep.name + "=" + sweep.values[k] + ": " + eqf_error_string(rc));
        }
    };
    // --warmup F: slot 0 alone, under the command line's settings, until F frames have run; then it is copied into the others, the sweep's values go to all
    // slots and the totals start again. Without a warm-up every slot runs from the start with its value.
    // `branched` and not live < B says whether that has happened: with B = 1 nothing is copied, yet the value, the reset and the count start at frame F too.
    int live = warmup > 0 ? 1 : B;
    bool branched = warmup == 0;
    auto branch = [&] {
        if (warm) { // the filter into all B slots, one call
            std::vector<int> all(B), st(B, 0);
            for (int k = 0; k < B; ++k)
                all[k] = k;
            check_rc(filters.loadFilter(*warm, B, all.data(), st.data()), "--warmupOnFilter: loading the filter into the slots");
            for (int k = 0; k < B; ++k)
                if (st[k] != 0)
                    throw std::runtime_error("--warmupOnFilter: loading the filter into slot " + std::to_string(k) + ": " + eqf_error_string(st[k]));
            warm.reset();
        } else {
            std::vector<int> src(B - 1, 0), dst(B - 1), st(B - 1, 0);
            for (int k = 1; k < B; ++k)
                dst[k - 1] = k;
            if (B > 1)
                filters.copySlots(B - 1, src.data(), dst.data(), st.data());
            for (int k = 1; k < B; ++k)
                if (st[k - 1] != 0)
                    throw std::runtime_error("--warmup: copying slot 0 into slot " + std::to_string(k) + ": " + eqf_error_string(st[k - 1]));
        }
        applySweep();
        if (!rechart.empty()) { // --rechart: every slot into its chart, one call; behind the sweep's settings, which carry the warm-up's chart
            std::vector<int> all(B), st(B, 0);
            for (int k = 0; k < B; ++k)
                all[k] = k;
            check_rc(filters.convertChart(B, all.data(), rechart.data(), st.data()), "--rechart");
            for (int k = 0; k < B; ++k)
                if (st[k] != 0)
                    throw std::runtime_error("--rechart: converting slot " + std::to_string(k) + ": " + eqf_error_string(st[k]));
        }
        check_rc(eqf_batch_reset_innovation_totals(filters.core(), -1), "eqf_batch_reset_innovation_totals");
        live = B;
        branched = true;
    };
    if (warmup == 0)
        applySweep();
    for (int k = 0; k < B && !charts.empty(); ++k) // behind the sweep's settings, which carry a chart of their own; no slot holds a landmark yet
        check_rc(filters.setChart(k, charts[k]), "--batchChart");
    std::vector<int> slots(B), status(B), failed(B, 0);
    for (int k = 0; k < B; ++k)
        slots[k] = k;
    int imuDataCounter = 0, visionDataCounter = 0, scoredFrames = 0;
    const auto loopStartTime = std::chrono::steady_clock::now();
    while (true) {
        const MeasurementType measType = dataServer.nextMeasurementType();
        if (measType == MeasurementType::None)
            break;
        if (measType == MeasurementType::Image) {
            const VisionMeasurement measData = dataServer.getSimVision();
            if (startTime > 0 && measData.stamp < startTime)
                continue;
            if (!branched && visionDataCounter == warmup)
                branch(); // before the first frame after the warm-up, and behind every IMU sample that came before it
            if (predictions && branched) { // where every live slot expects its landmarks at this stamp: one call, before the step
                std::fill(predCams.begin(), predCams.end(), measData.cameraPtr->c);
                std::fill(predStamps.begin(), predStamps.end(), measData.stamp);
                check_rc(filters.getFeaturePredictions(live, slots.data(), predCams.data(), predStamps.data(), predicted.data(), status.data()), "eqf_batch_predictions");
                for (int k = 0; k < live; ++k) {
                    check_rc(status[k], "eqf_batch_predictions");
                    const eqf_batch_prediction_record& r = predicted[k];
                    for (int i = 0; i < r.N; ++i) {
                        const auto it = measData.camCoordinates.find(r.ids[i]);
                        if (it == measData.camCoordinates.end())
                            continue;
                        const double du = r.y[2 * i] - it->second[0], dv = r.y[2 * i + 1] - it->second[1];
                        predSq[k] += du * du + dv * dv;
                        ++predCount[k];
                    }
                }
            }
            if (warm) { // a warm-up frame on the single filter: no slot runs, nothing is scored or recorded
                warm->processVisionData(measData);
                ++visionDataCounter;
                if (stopTime > 0 && warm->getTime() > stopTime)
                    break;
                continue;
            }
            const std::vector<const VisionMeasurement*> meas(B, &measData);
            filters.processVisionData(live, slots.data(), meas.data(), status.data()); // one device step for all live slots
            for (int k = 0; k < live; ++k) {
                if (status[k] == EQF_E_NOT_SPD || status[k] == EQF_E_NONFINITE) {
                    if (branched)
                        ++failed[k]; // this tuning's update failed on this frame: the slot goes on without it, the others are not affected
                } else if (status[k] != 0)
                    throw std::runtime_error("slot " + std::to_string(k) + ", stamp " + std::to_string(measData.stamp) + ": " + eqf_error_string(status[k]));
            }
            ++visionDataCounter;
            scoredFrames += branched;
            if (wantEstimates) {
                check_rc(eqf_batch_estimates(filters.core(), live, slots.data(), records.data(), status.data()), "eqf_batch_estimates");
                for (int k = 0; k < live; ++k) {
                    check_rc(status[k], "eqf_batch_estimates");
                    const eqf_batch_estimate_record& r = records[k];
                    const double stamp = filters.slot(k).currentTime; // -1 before the slot has initialised, as main() writes it
                    if (writers[k])
                        writeEstimateRecord(*writers[k], stamp, r);
                    if (groundtruth)
                        trajectories[k].push_back(StampedPose{stamp, Pose{Qt{r.sensor[6], r.sensor[7], r.sensor[8], r.sensor[9]}, V3{r.sensor[10], r.sensor[11], r.sensor[12]}}});
                }
            }
        } else {
            const IMUVelocity imuData = dataServer.getIMU();
            if (startTime > 0 && imuData.stamp < startTime)
                continue;
            if (warm)
                warm->processIMUData(imuData);
            for (int k = 0; k < live && !warm; ++k)
                filters.processIMUData(k, imuData);
            ++imuDataCounter;
        }
        if (stopTime > 0 && (warm ? warm->getTime() : filters.slot(0).currentTime) > stopTime)
            break;
    }
    const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopStartTime).count();
    std::cout << "Processed " << imuDataCounter << " IMU and " << visionDataCounter << " vision measurements in " << B << " slots.\n"
              << "Time taken: " << elapsed << " seconds." << std::endl;
    if (warmup > 0) {
        if (!branched)
            throw std::runtime_error("--warmup " + std::to_string(warmup) + ": the sequence has only " + std::to_string(visionDataCounter) + " vision frames");
        if (warmupOnFilter)
            std::printf("warm-up: %d frames on a single filter, then loaded into %d slots; scores over the %d frames after the warm-up\n", warmup, B, scoredFrames);
        else
            std::printf("warm-up: %d frames in slot 0, then copied into %d slots; scores over the %d frames after the warm-up\n", warmup, B - 1, scoredFrames);
    }
    for (int k = 0; k < B; ++k) {
        const VIOFilterBatch::InnovationTotals t = filters.innovationTotals(k);
        const std::string what = label(k);
        std::printf("slot %d%s: frames updated %ld  failed %d  mean NIS/dof %.9g  log-likelihood %.9g\n", k, what.c_str(), t.updates, failed[k], t.meanNisPerDof(),
                    t.logLikelihood());
    }
    for (int k = 0; k < B && groundtruth; ++k) {
        const TrajectoryScore t = trajectoryPositionRMSE(trajectories[k], *groundtruth);
        const std::string what = label(k);
        std::printf("slot %d%s: position RMSE %.9g over %d frames\n", k, what.c_str(), t.rmse, t.frames);
    }
    for (int k = 0; k < B && predictions; ++k) {
        const std::string what = label(k);
        std::printf("slot %d%s: prediction RMSE %.9g px over %ld features\n", k, what.c_str(), std::sqrt(predSq[k] / (double)predCount[k]), predCount[k]);
    }
    std::printf("batch of %d slots: slots x vision updates/s %.1f\n", B, (double)B * visionDataCounter / elapsed);
    return 0;
}

int main(int argc, char** argv) {
    VIOFilter::Settings fs;
    std::string imuName, featName, gtName, outputDir, cameraFileName, statesName, recordDir;
    DatasetFormat format = DatasetFormat::ASL;
    auto cam = std::make_shared<Camera>();
    cam->c.fx = 458.654; // intrinsics.yaml:7 (EuRoC cam0)
    cam->c.fy = 457.296;
    cam->c.cx = 367.215;
    cam->c.cy = 248.375;
    cam->c.width = 752;
    cam->c.height = 480;
    double cameraLag = 0, startTime = -1, stopTime = -1;
    bool quiet = false, dump = false, sigmaFP32 = false, printCamera = false, haveSweep = false, haveWarmup = false, predictions = false, warmupOnFilter = false, nisLine = false;
    int batch = 0;
    std::string warmupText, riccatiText, chartText, rechartText, branchAtText, branchChartsText;
    bool haveRiccati = false, haveChart = false, haveRechart = false, haveBranchAt = false, haveBranchCharts = false;
    std::vector<int> riccati, charts, rechart, branchCharts;
    int branchAt = 0;
    Sweep sweep;
    try {
        for (int i = 1; i < argc; ++i) {
            const std::string a = argv[i];
            std::function<const char*()> val = [&]() -> const char* {
                if (i + 1 >= argc)
                    throw std::runtime_error("missing value after " + a);
                return argv[++i];
            };
            if (a == "--imu") imuName = val();
            else if (a == "--features") featName = val();
            else if (a == "--groundtruth") gtName = val();
            else if (a == "--cameraFile") cameraFileName = val();
            else if (a == "--dumpStates") statesName = val();
            else if (a == "--format") {
                const std::string f = val();
                if (f == "asl") format = DatasetFormat::ASL;
                else if (f == "uzhfpv") format = DatasetFormat::UZHFPV;
                else throw std::runtime_error("unknown --format " + f);
            } else if (a == "--camera") {
                cam->c.fx = std::atof(val());
                cam->c.fy = std::atof(val());
                cam->c.cx = std::atof(val());
                cam->c.cy = std::atof(val());
                cam->c.width = std::atoi(val());
                cam->c.height = std::atoi(val());
            } else if (a == "--distortion") { // radtan k1 k2 p1 p2 k3 (sensor.yaml distortion_coefficients) | equidistant k1 k2 k3 k4
                const std::string mdl = val();
                if (mdl == "radtan") {
                    cam->c.model = EQVIO_CAMERA_RADTAN;
                    for (int k = 0; k < 5; ++k)
                        cam->c.dist[k] = std::atof(val());
                } else if (mdl == "equidistant") {
                    cam->c.model = EQVIO_CAMERA_EQUIDISTANT;
                    for (int k = 0; k < 4; ++k)
                        cam->c.dist[k] = std::atof(val());
                } else
                    throw std::runtime_error("unknown --distortion model " + mdl + " (radtan | equidistant)");
            } else if (a == "--cameraOffset") {
                double q[7];
                for (double& v : q)
                    v = std::atof(val());
                fs.cameraOffset = Pose{eqf::q_unit(Qt{q[0], q[1], q[2], q[3]}), V3{q[4], q[5], q[6]}};
            } else if (a == "--cameraLag") cameraLag = std::atof(val());
            else if (a == "--start") startTime = std::atof(val());
            else if (a == "--stop") stopTime = std::atof(val());
            else if (a == "--output") outputDir = val();
            else if (a == "--quiet") quiet = true;
            else if (a == "--sigmaFP32") sigmaFP32 = true;
            else if (a == "--dumpMeasurements") dump = true;
            else if (a == "--printCamera") printCamera = true;
            else if (a == "--batch") batch = std::atoi(val());
            else if (a == "--record") recordDir = val();
            else if (a == "--predictions") predictions = true;
            else if (a == "--nis") nisLine = true;
            else if (a == "--warmupOnFilter") warmupOnFilter = true;
            else if (a == "--batchRiccati") {
                riccatiText = val();
                haveRiccati = true;
            } else if (a == "--batchChart") {
                chartText = val();
                haveChart = true;
            } else if (a == "--rechart") {
                rechartText = val();
                haveRechart = true;
            }
            else if (a == "--branchAt") {
                branchAtText = val();
                haveBranchAt = true;
            } else if (a == "--branchCharts") {
                branchChartsText = val();
                haveBranchCharts = true;
            }
            else if (a == "--sweep") {
                sweep = parseSweep(val());
                haveSweep = true;
            } else if (a == "--warmup") {
                warmupText = val();
                haveWarmup = true;
            }
            else if (!parseFilterFlag(a, val, fs)) {
                usage();
                return a == "--help" ? 0 : 2;
            }
        }
        if (nisLine && batch != 0) { // before any file or device is opened
            std::fprintf(stderr, "eqvio_opt: --nis is the single filter's score; with --batch B every slot's line carries it already\n");
            return 2;
        }
        if (haveBranchAt || haveBranchCharts) { // before any file or device is opened
            std::string refusal = branchRefusal(haveBranchAt, branchAtText, haveBranchCharts, branchChartsText, batch, branchAt, branchCharts);
            if (refusal.empty())
                refusal = !outputDir.empty() ? "--branchAt does not support --output" : !statesName.empty() ? "--branchAt does not support --dumpStates"
                          : sigmaFP32 ? "--branchAt does not support --sigmaFP32 (the float Sigma store is neither copied nor converted)" : "";
            if (!refusal.empty()) {
                std::fprintf(stderr, "eqvio_opt: %s\n", refusal.c_str());
                return 2;
            }
        }
        if (haveSweep && batch == 0) {
            std::fprintf(stderr, "eqvio_opt: --sweep needs --batch B (one value per slot)\n");
            return 2;
        }
        if (!recordDir.empty() && batch == 0) { // before any file or device is opened
            std::fprintf(stderr, "eqvio_opt: --record needs --batch\n");
            return 2;
        }
        if (predictions && batch == 0) { // before any file or device is opened
            std::fprintf(stderr, "eqvio_opt: --predictions needs --batch\n");
            return 2;
        }
        if (predictions)
            fs.useFeaturePredictions = true;
        if (haveRiccati) { // before any file or device is opened
            const std::string refusal = batchRiccatiRefusal(riccatiText, batch < 0 ? 0 : batch, riccati);
            if (!refusal.empty()) {
                std::fprintf(stderr, "eqvio_opt: %s\n", refusal.c_str());
                return 2;
            }
            fs.fastRiccati = true; // the batch's settings describe eqf_batch_step; the modes go to the slots
        }
        if (haveChart) { // before any file or device is opened
            const std::string refusal = batchChartRefusal(chartText, batch < 0 ? 0 : batch, charts);
            if (!refusal.empty()) {
                std::fprintf(stderr, "eqvio_opt: %s\n", refusal.c_str());
                return 2;
            }
        }
        if (haveRechart) { // before any file or device is opened
            const std::string refusal = rechartRefusal(rechartText, batch < 0 ? 0 : batch, haveChart, sweep, rechart);
            if (!refusal.empty()) {
                std::fprintf(stderr, "eqvio_opt: %s\n", refusal.c_str());
                return 2;
            }
        }
        int warmup = 0;
        if (haveWarmup) { // before any file or device is opened, as the refusals of --batch
            char* end = nullptr;
            const long f = std::strtol(warmupText.c_str(), &end, 10);
            const std::string why = batch == 0 || (!haveSweep && !haveRechart) ? "needs --batch B and --sweep NAME=v0,... or --rechart C,... (the warm-up is what the slots branch from)"
                                    : warmupText.empty() || *end ? "'" + warmupText + "' is not a number of frames"
                                    : f < 0 ? "needs F >= 0"
                                    : f > 1000000000 ? "is more frames than any sequence has"
                                    : "";
            if (!why.empty()) {
                std::fprintf(stderr, "eqvio_opt: --warmup %s: %s\n", warmupText.c_str(), why.c_str());
                return 2;
            }
            warmup = (int)f;
        }
        if (haveRechart && !rechartWarmupRefusal(warmup).empty()) { // before any file or device is opened
            std::fprintf(stderr, "eqvio_opt: %s\n", rechartWarmupRefusal(warmup).c_str());
            return 2;
        }
        if (warmupOnFilter && warmup == 0) { // before any file or device is opened
            std::fprintf(stderr, "eqvio_opt: --warmupOnFilter needs --warmup F with F > 0 (it says where the warm-up's frames run)\n");
            return 2;
        }
        if (batch != 0) { // what the filter batch refuses, before any file or device is opened
            std::string why = batch < 1 ? "needs B >= 1"
                              : !fs.fastRiccati ? "needs --fastRiccati 1 (the batch has fast Riccati only; the default is 0)"
                              : !outputDir.empty() ? "does not support --output"
                              : !statesName.empty() ? "does not support --dumpStates"
                              : sigmaFP32 ? "does not support --sigmaFP32"
                              : "";
            if (why.empty() && haveSweep)
                why = sweepRefusal(sweep, batch, batchSettings(fs));
            if (why.empty() && warmup > 0 && haveSweep)
                why = warmupSweepRefusal(sweep);
            if (why.empty() && haveSweep && haveChart)
                why = batchChartSweepRefusal(sweep);
            if (why.empty() && warmup > 0 && haveChart)
                why = "--warmup with --batchChart: the chart cannot change under a filter that holds landmarks";
            if (!why.empty()) {
                std::fprintf(stderr, "eqvio_opt: --batch %d: %s\n", batch, why.c_str());
                return 2;
            }
        }
        if (imuName.empty() || featName.empty()) {
            usage();
            return 2;
        }
        if (!cameraFileName.empty()) // after the flags: --format decides which layout the file has (main_opt.cpp:114-147)
            readCameraFile(cameraFileName, format, *cam, fs.cameraOffset);
        if (printCamera) { // host-only: the camera and the camera offset as the run would use them (model fx fy cx cy width height k1..k5 | qw qx qy qz x y z)
            std::printf("camera %d %.17g %.17g %.17g %.17g %d %d %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", cam->c.model, cam->c.fx, cam->c.fy, cam->c.cx,
                        cam->c.cy, cam->c.width, cam->c.height, cam->c.dist[0], cam->c.dist[1], cam->c.dist[2], cam->c.dist[3], cam->c.dist[4], fs.cameraOffset.R.w, fs.cameraOffset.R.x,
                        fs.cameraOffset.R.y, fs.cameraOffset.R.z, fs.cameraOffset.x.x, fs.cameraOffset.x.y, fs.cameraOffset.x.z);
            return 0;
        }
        TrackReplayServer dataServer(imuName, featName, format, cam, cameraLag);
        if (dump) { // host-only: print the merged measurement stream as parsed (no filter, no device)
            std::printf("%s", "");
            while (dataServer.nextMeasurementType() != MeasurementType::None) {
                const double t = dataServer.nextTime();
                if (dataServer.nextMeasurementType() == MeasurementType::IMU) {
                    const IMUVelocity v = dataServer.getIMU();
                    std::printf("IMU %.17g %.17g %.17g %.17g %.17g %.17g %.17g\n", v.stamp, v.gyr.x, v.gyr.y, v.gyr.z, v.acc.x, v.acc.y, v.acc.z);
                    if (v.stamp != t)
                        throw std::runtime_error("nextTime disagrees with the IMU stamp");
                } else {
                    const VisionMeasurement m = dataServer.getSimVision();
                    std::printf("IMG %.17g %zu", m.stamp, m.camCoordinates.size());
                    for (const auto& kv : m.camCoordinates)
                        std::printf(" %d %.17g %.17g", kv.first, kv.second[0], kv.second[1]);
                    std::printf("\n");
                }
            }
            if (!gtName.empty()) {
                const std::vector<StampedPose> gt = TrackReplayServer::groundtruth(gtName, format);
                std::printf("GT %zu", gt.size());
                if (!gt.empty())
                    std::printf(" %.17g %.17g %.17g %.17g %.17g %.17g %.17g %.17g", gt[0].t, gt[0].pose.x.x, gt[0].pose.x.y, gt[0].pose.x.z, gt[0].pose.R.w, gt[0].pose.R.x,
                                gt[0].pose.R.y, gt[0].pose.R.z);
                std::printf("\n");
            }
            return 0;
        }
        if (batch != 0) {
            std::vector<StampedPose> gt;
            if (!gtName.empty())
                gt = TrackReplayServer::groundtruth(gtName, format);
            return runBatch(dataServer, fs, batch, sweep, warmup, startTime, stopTime, recordDir, gtName.empty() ? nullptr : &gt, predictions, warmupOnFilter, riccati, charts, rechart);
        }
        loopTimer.initialise({"correction", "features", "preprocessing", "propagation", "total", "total vision update", "write output"});
        VIOFilter filter(fs); // main_opt.cpp:150
        if (sigmaFP32) // BASELINE config 5: Sigma stored as float in HBM (include/eqf_hip.h)
            eqf_set_option(filter.eqfState().ctx, EQF_OPT_SIGMA_FP32, 2);
        if (nisLine)
            filter.setInnovationStats(true);
        std::unique_ptr<VIOWriter> vioWriter;
        if (!outputDir.empty())
            vioWriter = std::make_unique<VIOWriter>(outputDir);
        // --dumpStates: the state estimate after every vision measurement at FULL precision (%.17g; the writer's files carry 6 digits), one line per frame:
        // time, the 23 numbers of the sensor state (bias, pose wxyz + xyz, velocity, camera offset), N, then id x y z per landmark. For parity tests.
        std::FILE* statesFile = statesName.empty() ? nullptr : std::fopen(statesName.c_str(), "w");
        if (!statesName.empty() && !statesFile)
            throw std::runtime_error("cannot open " + statesName);
        int imuDataCounter = 0, visionDataCounter = 0;
        // --branchAt F: empty until F frames have run; then one filter per chart, each a converted copy of `filter`, which runs no further frame
        std::vector<std::unique_ptr<VIOFilter>> branches;
        auto branch = [&] {
            for (const int chart : branchCharts) {
                auto b = std::make_unique<VIOFilter>(fs); // fresh, in the warm-up's chart: its innovation totals count the frames after the branch
                if (nisLine)
                    b->setInnovationStats(true);
                b->copyFrom(filter);
                b->convertChart(chart);
                branches.push_back(std::move(b));
            }
        };
        const auto loopStartTime = std::chrono::steady_clock::now();
        while (true) {
            const MeasurementType measType = dataServer.nextMeasurementType();
            if (measType == MeasurementType::None)
                break;
            if (measType == MeasurementType::Image) {
                loopTimer.startLoop();
                loopTimer.startTiming("total");
                VisionMeasurement measData = dataServer.getSimVision();
                if (startTime > 0 && measData.stamp < startTime)
                    continue;
                if (branchAt > 0 && branches.empty() && visionDataCounter == branchAt)
                    branch(); // before the first frame after the warm-up, and behind every IMU sample that came before it
                if (!branches.empty()) {
                    for (auto& b : branches)
                        b->processVisionData(measData);
                    ++visionDataCounter;
                    if (stopTime > 0 && branches[0]->getTime() > stopTime)
                        break;
                    continue;
                }
                loopTimer.startTiming("total vision update");
                filter.processVisionData(measData);
                loopTimer.endTiming("total vision update");
                loopTimer.endTiming("total");
                ++visionDataCounter;
                loopTimer.startTiming("write output");
                const VIOState estimatedState = filter.stateEstimate();
                if (statesFile) {
                    const VIOSensorState& se = estimatedState.sensor;
                    std::fprintf(statesFile, "%.17g", filter.getTime());
                    const double sv[23] = {se.inputBias[0], se.inputBias[1], se.inputBias[2], se.inputBias[3], se.inputBias[4], se.inputBias[5], se.pose.R.w, se.pose.R.x, se.pose.R.y,
                                           se.pose.R.z, se.pose.x.x, se.pose.x.y, se.pose.x.z, se.velocity.x, se.velocity.y, se.velocity.z, se.cameraOffset.R.w, se.cameraOffset.R.x,
                                           se.cameraOffset.R.y, se.cameraOffset.R.z, se.cameraOffset.x.x, se.cameraOffset.x.y, se.cameraOffset.x.z};
                    for (const double v : sv)
                        std::fprintf(statesFile, " %.17g", v);
                    std::fprintf(statesFile, " %zu", estimatedState.cameraLandmarks.size());
                    for (const Landmark& lm : estimatedState.cameraLandmarks)
                        std::fprintf(statesFile, " %d %.17g %.17g %.17g", lm.id, lm.p.x, lm.p.y, lm.p.z);
                    std::fprintf(statesFile, "\n");
                }
                if (vioWriter) {
                    vioWriter->writeStates(filter.getTime(), estimatedState);
                    vioWriter->writeFeatures(measData);
                }
                loopTimer.endTiming("write output");
                if (vioWriter)
                    vioWriter->writeTiming(loopTimer.getLoopTimingData());
            } else {
                const IMUVelocity imuData = dataServer.getIMU();
                if (startTime > 0 && imuData.stamp < startTime)
                    continue;
                if (branches.empty())
                    filter.processIMUData(imuData);
                for (auto& b : branches)
                    b->processIMUData(imuData);
                ++imuDataCounter;
            }
            if (stopTime > 0 && (branches.empty() ? filter : *branches[0]).getTime() > stopTime)
                break;
        }
        const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopStartTime).count();
        if (statesFile)
            std::fclose(statesFile);
        std::cout << "Processed " << imuDataCounter << " IMU and " << visionDataCounter << " vision measurements.\n"
                  << "Time taken: " << elapsed << " seconds." << std::endl;
        if (branchAt > 0) { // every branch's lines, labelled with its chart: what the single filter prints, over the frames after the branch
            if (branches.empty())
                throw std::runtime_error("--branchAt " + std::to_string(branchAt) + ": the sequence has only " + std::to_string(visionDataCounter) + " vision frames");
            std::printf("branch: %d frames on a single filter (chart %s), then copied into %zu filters and converted; scores over the %d frames after the branch\n", branchAt,
                        batchChartName((int)fs.coordinateChoice), branches.size(), visionDataCounter - branchAt);
            std::vector<StampedPose> gt;
            if (!gtName.empty())
                gt = TrackReplayServer::groundtruth(gtName, format);
            for (size_t k = 0; k < branches.size(); ++k) {
                VIOFilter& b = *branches[k];
                const std::string what = "branch " + std::to_string(k) + " chart " + batchChartName(branchCharts[k]);
                const VIOState est = b.stateEstimate();
                std::printf("%s: final time %.9g  position %.9g %.9g %.9g  landmarks %d\n", what.c_str(), b.getTime(), est.sensor.pose.x.x, est.sensor.pose.x.y, est.sensor.pose.x.z,
                            b.viewEqFState().numLandmarks());
                if (nisLine) {
                    long updates = 0, dof = 0;
                    double nis = 0, logdet = 0;
                    b.innovationTotals(updates, dof, nis, logdet);
                    std::printf("%s: frames updated %ld  mean NIS/dof %.9g  log-likelihood %.9g\n", what.c_str(), updates, nis / (double)dof,
                                -0.5 * (nis + logdet + (double)dof * std::log(2.0 * M_PI)));
                }
                if (!gt.empty()) { // distance to the ground-truth pose nearest in time
                    size_t j = 0;
                    for (size_t i = 0; i < gt.size(); ++i)
                        if (std::fabs(gt[i].t - b.getTime()) < std::fabs(gt[j].t - b.getTime()))
                            j = i;
                    const V3 d{est.sensor.pose.x.x - gt[j].pose.x.x, est.sensor.pose.x.y - gt[j].pose.x.y, est.sensor.pose.x.z - gt[j].pose.x.z};
                    std::printf("%s: groundtruth poses %zu  nearest stamp %.9g  position %.6g %.6g %.6g  distance %.9g\n", what.c_str(), gt.size(), gt[j].t, gt[j].pose.x.x,
                                gt[j].pose.x.y, gt[j].pose.x.z, std::sqrt(d.x * d.x + d.y * d.y + d.z * d.z));
                }
            }
            return 0;
        }
        const VIOState est = filter.stateEstimate();
        std::printf("final time %.9g  position %.6g %.6g %.6g  landmarks %d  vision updates/s %.1f\n", filter.getTime(), est.sensor.pose.x.x, est.sensor.pose.x.y,
                    est.sensor.pose.x.z, filter.viewEqFState().numLandmarks(), visionDataCounter / elapsed);
        if (nisLine) { // the wording of --batch B's per-slot line
            long updates = 0, dof = 0;
            double nis = 0, logdet = 0;
            filter.innovationTotals(updates, dof, nis, logdet);
            std::printf("single filter: frames updated %ld  mean NIS/dof %.9g  log-likelihood %.9g\n", updates, nis / (double)dof, -0.5 * (nis + logdet + (double)dof * std::log(2.0 * M_PI)));
        }
        if (!gtName.empty()) { // distance to the ground-truth pose nearest in time, after aligning the first poses
            const std::vector<StampedPose> gt = TrackReplayServer::groundtruth(gtName, format);
            if (!gt.empty()) {
                size_t k = 0;
                for (size_t j = 0; j < gt.size(); ++j)
                    if (std::fabs(gt[j].t - filter.getTime()) < std::fabs(gt[k].t - filter.getTime()))
                        k = j;
                std::printf("groundtruth poses %zu  nearest stamp %.9g  position %.6g %.6g %.6g\n", gt.size(), gt[k].t, gt[k].pose.x.x, gt[k].pose.x.y, gt[k].pose.x.z);
            }
        }
        (void)quiet;
    } catch (const std::exception& e) {
        std::fprintf(stderr, "eqvio_opt: %s\n", e.what());
        return 1;
    }
    return 0;
}
