// eqvio_sim: the reference's simulation main (src/main_sim.cpp:128-184) on the MI355X EqF path.
// Same loop: Image -> [augmentLandmarkStates] -> processVisionData -> stateEstimate / computeNEES / write;
// IMU -> processIMUData -> optional landmark reset. Configuration comes from --key value flags instead of a YAML file
// (yaml-cpp and argparse are not in this image); defaults are the reference's.
#include "VIOSimulator.hpp"
#include "VIOWriter.hpp"
#include "cli.hpp"
#include "eqvio_batch.h"
#include <algorithm>
#include <fstream>
#include <iomanip>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>

using namespace eqvio_amd;

static void usage() {
    std::puts("usage: eqvio_sim [--duration S] [--trajectory wave|square|sine|line] [--numPoints N] [--numWalls W] [--wallDistance D]\n"
              "                 [--maxFeatures M] [--seed S] [--imuFreq HZ] [--imageFreq HZ] [--initialNoise] [--inputNoise] [--outputNoise]\n"
              "                 [--fullState] [--landmarkReset S] [--output DIR] [--writeDataset DIR] [--sigmaFP32] [--quiet] [--batch B]\n"
              "                 [--sweep NAME=v0,v1,...] [--innovation] [--nis] [--record DIR] [--batchRiccati fast|accurate|discrete[,...]]\n"
              "                 [--batchChart euclidean|invdepth|normal[,...]]\n"
              "                 [--<eqf setting> VALUE ...]   (names of VIOFilter::Settings, e.g. --fastRiccati 1 --coordinateChoice InvDepth)\n"
              "  --batch B   runs the seeds --seed .. --seed + B - 1 as B slots of one filter batch (include/eqvio_batch.h) and prints each run's mean\n"
              "              NEES and their mean. The batch needs fast Riccati, which is not the default: give --fastRiccati 1 (the setting of the\n"
              "              shipped EuRoC / UZH-FPV configurations); the Normal chart, --maxFeatures above 64, --fullState, --landmarkReset and\n"
              "              --output are refused.\n"
              "  --sweep NAME=v0,...,v(B-1)   with --batch B: runs the SAME seed (--seed) in every slot, slot k with the filter setting NAME (a field of\n"
              "              eqvio_settings: doubles, the 0 / 1 flags, coordinateChoice as Euclidean|InvDepth) at value vk, and prints each run's value and\n"
              "              mean NEES. The simulated data are those of the unswept settings. Needs exactly B values.\n"
              "  --innovation   with --batch B: behind those lines, one line per run with the number of vision updates, the mean normalised innovation\n"
              "              squared per degree of freedom (sum NIS / sum dof: about 1 for a consistent filter) and the total innovation log-likelihood\n"
              "              (eqvio_batch_innovation_totals). Needs no true state, unlike NEES.\n"
              "  --nis   a single run (no --batch): switches the device context's innovation statistics on (EQF_OPT_INNOVATION_STATS) and prints, after the run,\n"
              "              the number of vision updates, the mean NIS per degree of freedom and the total innovation log-likelihood, in --innovation's wording\n"
              "  --record DIR   with --batch B: writes every run's consistency record to DIR/run_<k>/ - nees.csv (NEES, PoseNEES, AttitudeNEES),\n"
              "              poseConsistency.csv, cameraConsistency.csv, biasConsistency.csv and landmarkError.csv, in the formats of --output - from one\n"
              "              launch per frame for all runs (eqvio_batch_run_sim_recorded).\n"
              "  --batchRiccati M[,M...]   with --batch B: the runs' propagation, M = fast (one fast Riccati step per frame), accurate (the reference's\n"
              "              default, fastRiccati: false: one accurate Riccati step per IMU sample) or discrete (accurate with the discrete state matrix,\n"
              "              useDiscreteStateMatrix: true); one value for every run, or B values, one per run.\n"
              "              With this flag --fastRiccati 1 need not be given: the tool hands the batch that setting itself. Each run's line names its mode.\n"
              "  --batchChart C[,C...]   with --batch B: the runs' coordinate chart, C = euclidean, invdepth or normal (the reference's third chart, which\n"
              "              --coordinateChoice and --sweep coordinateChoice=... do not take with --batch); one value for every run, or B values, one per run.\n"
              "              Combines with --batchRiccati and --sweep. Each run's line names its chart.");
}

// --batch B: the default-mode loop of main() for B seeds in lockstep, through eqvio_batch_run_sim (augment, vision step and NEES: one launch each per frame)
static int runBatch(const SimSettings& sim, const VIOFilter::Settings& fs, int B, bool quiet, const Sweep& sweep, bool innovation, const std::string& recordDir,
                    const std::vector<int>& riccati, const std::vector<int>& charts) {
    const bool swept = !sweep.name.empty();
    eqvio_sim_settings ss;
    eqvio_sim_default_settings(&ss);
    ss.numPoints = sim.numPoints;
    ss.wallDistance = sim.wallDistance;
    ss.numWalls = sim.numWalls;
    ss.maxFeatures = (int)sim.maxFeatures;
    ss.initialNoise = sim.initialNoise, ss.inputNoise = sim.inputNoise, ss.outputNoise = sim.outputNoise;
    ss.duration = sim.duration;
    const char* names[4] = {"wave", "square", "sine", "line"};
    ss.trajectory = (int)(std::find(names, names + 4, sim.trajectory) - names);
    ss.imuFreq = sim.imuFreq;
    ss.imageFreq = sim.imageFreq;
    eqvio_settings es = batchSettings(fs);
    std::vector<eqvio_sim*> sims(B, nullptr);
    auto release = [&] {
        for (eqvio_sim* s : sims)
            eqvio_sim_destroy(s);
    };
    for (int k = 0; k < B; ++k) {
        ss.randomSeed = sim.randomSeed + (swept ? 0u : (unsigned)k); // a sweep runs the same seed in every slot
        sims[k] = eqvio_sim_create(&ss, &es);
        if (!sims[k]) {
            std::fprintf(stderr, "eqvio_sim: eqvio_sim_create failed\n");
            release();
            return 1;
        }
    }
    eqvio_sim_camera_offset(sims[0], es.cameraOffset); // camera extrinsics of the data server (main_sim.cpp:97-101)
    eqvio_batch* b = nullptr;
    int rc = eqvio_batch_create(&b, &es, fs.device, B, (int)sim.maxFeatures);
    if (rc) {
        std::fprintf(stderr, "eqvio_sim: eqvio_batch_create: %s\n", eqf_error_string(rc));
        release();
        return 1;
    }
    for (int k = 0; k < B && swept; ++k) { // slot k: the batch's settings with the swept field at its k-th value
        eqvio_settings ek = es;
        std::string why;
        setSettingsField(ek, sweep.name, sweep.values[k], why);
        rc = eqvio_batch_set_slot_settings(b, k, &ek);
        if (rc) {
            std::fprintf(stderr, "eqvio_sim: --sweep %s=%s: %s\n", sweep.name.c_str(), sweep.values[k].c_str(), rc == -1 ? eqvio_batch_last_error(b) : eqf_error_string(rc));
            eqvio_batch_destroy(b);
            release();
            return 1;
        }
    }
    for (int k = 0; k < B && !riccati.empty(); ++k)
        if ((rc = eqvio_batch_set_slot_riccati(b, k, batchCliRiccati(riccati[k]))) || (rc = eqvio_batch_set_slot_state_matrix(b, k, batchCliStateMatrix(riccati[k])))) {
            std::fprintf(stderr, "eqvio_sim: --batchRiccati: slot %d: %s\n", k, eqf_error_string(rc));
            eqvio_batch_destroy(b);
            release();
            return 1;
        }
    for (int k = 0; k < B && !charts.empty(); ++k) // behind the sweep's settings, which carry a chart of their own; the slots hold no landmark yet
        if ((rc = eqvio_batch_set_slot_chart(b, k, charts[k]))) {
            std::fprintf(stderr, "eqvio_sim: --batchChart: slot %d: %s\n", k, eqf_error_string(rc));
            eqvio_batch_destroy(b);
            release();
            return 1;
        }
    const int maxFrames = (int)std::ceil(sim.duration * sim.imageFreq) + 2;
    std::vector<double> nees((size_t)maxFrames * B);
    int frames = 0;
    const auto t0 = std::chrono::steady_clock::now();
    rc = recordDir.empty() ? eqvio_batch_run_sim(b, sims.data(), maxFrames, nees.data(), &frames)
                           : eqvio_batch_run_sim_recorded(b, sims.data(), maxFrames, nees.data(), &frames, recordDir.c_str());
    const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rc) {
        std::fprintf(stderr, "eqvio_sim: %s: %s\n", recordDir.empty() ? "eqvio_batch_run_sim" : "eqvio_batch_run_sim_recorded", rc == -1 ? eqvio_batch_last_error(b) : eqf_error_string(rc));
        eqvio_batch_destroy(b);
        release();
        return 1;
    }
    double sumOfMeans = 0;
    for (int k = 0; k < B; ++k) {
        double s = 0;
        int n = 0;
        for (int j = 0; j < frames; ++j) {
            const double v = nees[(size_t)j * B + k];
            if (v == v)
                s += v, ++n;
        }
        const double mean = s / std::max(n, 1);
        sumOfMeans += mean;
        const std::string mode = (riccati.empty() ? std::string() : std::string(" riccati ") + batchRiccatiName(riccati[k])) +
                                 (charts.empty() ? std::string() : std::string(" chart ") + batchChartName(charts[k]));
        if (swept)
            std::printf("run %d seed %u %s=%s%s: mean NEES %.9g over %d frames\n", k, sim.randomSeed, sweep.name.c_str(), sweep.values[k].c_str(), mode.c_str(), mean, n);
        else
            std::printf("run %d seed %u%s: mean NEES %.9g over %d frames\n", k, sim.randomSeed + (unsigned)k, mode.c_str(), mean, n);
    }
    std::printf("batch of %d runs: mean of the runs' mean NEES %.9g  frames %d  runs x frames/s %.1f\n", B, sumOfMeans / B, frames, (double)B * frames / elapsed);
    for (int k = 0; k < B && innovation; ++k) { // the slot's totals over the whole run: every slot starts with none
        long updates = 0, dof = 0;
        double nis = 0, logdet = 0;
        eqvio_batch_innovation_totals(b, k, &updates, &dof, &nis, &logdet);
        std::printf("innovation run %d: updates %ld  mean NIS/dof %.9g  log-likelihood %.9g\n", k, updates, nis / (double)dof,
                    -0.5 * (nis + logdet + (double)dof * std::log(2.0 * M_PI)));
    }
    eqvio_batch_destroy(b);
    release();
    return 0;
}

int main(int argc, char** argv) {
    SimSettings sim;
    sim.duration = 20.0;
    VIOFilter::Settings fs;
    bool fullState = false, quiet = false, sigmaFP32 = false, innovation = false, nisLine = false;
    double landmarkResetTime = -1.0;
    int batch = 0;
    Sweep sweep;
    bool haveSweep = false;
    std::string outputDir, datasetDir, recordDir, riccatiText, chartText;
    bool haveRiccati = false, haveChart = false;
    std::vector<int> riccati, charts;
    for (int i = 1; i < argc; ++i) {
        const std::string a = argv[i];
        std::function<const char*()> val = [&]() -> const char* {
            if (i + 1 >= argc) {
                usage();
                std::exit(2);
            }
            return argv[++i];
        };
        if (a == "--duration") sim.duration = std::atof(val());
        else if (a == "--trajectory") sim.trajectory = val();
        else if (a == "--numPoints") sim.numPoints = std::atoi(val());
        else if (a == "--numWalls") sim.numWalls = std::atoi(val());
        else if (a == "--wallDistance") sim.wallDistance = std::atof(val());
        else if (a == "--maxFeatures") sim.maxFeatures = (size_t)std::atoi(val());
        else if (a == "--seed") sim.randomSeed = (uint32_t)std::strtoul(val(), nullptr, 10);
        else if (a == "--imuFreq") sim.imuFreq = std::atof(val());
        else if (a == "--imageFreq") sim.imageFreq = std::atof(val());
        else if (a == "--initialNoise") sim.initialNoise = true;
        else if (a == "--inputNoise") sim.inputNoise = true;
        else if (a == "--outputNoise") sim.outputNoise = true;
        else if (a == "--fullState") fullState = true;
        else if (a == "--landmarkReset") landmarkResetTime = std::atof(val());
        else if (a == "--output") outputDir = val();
        else if (a == "--writeDataset") datasetDir = val();
        else if (a == "--quiet") quiet = true;
        else if (a == "--sigmaFP32") sigmaFP32 = true;
        else if (a == "--batch") batch = std::atoi(val());
        else if (a == "--innovation") innovation = true;
        else if (a == "--nis") nisLine = true;
        else if (a == "--record") recordDir = val();
        else if (a == "--batchRiccati") {
            riccatiText = val();
            haveRiccati = true;
        }
        else if (a == "--batchChart") {
            chartText = val();
            haveChart = true;
        }
        else if (a == "--sweep") {
            sweep = parseSweep(val());
            haveSweep = true;
        }
        else if (parseFilterFlag(a, val, fs)) {
        } else {
            usage();
            return a == "--help" ? 0 : 2;
        }
    }
    if (haveSweep && batch == 0) {
        std::fprintf(stderr, "eqvio_sim: --sweep needs --batch B (one value per slot)\n");
        return 2;
    }
    if (nisLine && batch != 0) { // before any device is opened
        std::fprintf(stderr, "eqvio_sim: --nis is the single filter's score; with --batch B the filter batch reports it (--innovation)\n");
        return 2;
    }
    if (innovation && batch == 0) {
        std::fprintf(stderr, "eqvio_sim: --innovation needs --batch B (the statistics are the filter batch's)\n");
        return 2;
    }
    if (!recordDir.empty() && batch == 0) {
        std::fprintf(stderr, "eqvio_sim: --record needs --batch B (the records are the filter batch's; a single run writes them with --output)\n");
        return 2;
    }
    if (haveRiccati) { // before any device is opened
        const std::string refusal = batchRiccatiRefusal(riccatiText, batch < 0 ? 0 : batch, riccati);
        if (!refusal.empty()) {
            std::fprintf(stderr, "eqvio_sim: %s\n", refusal.c_str());
            return 2;
        }
        fs.fastRiccati = true; // the batch's settings describe eqf_batch_step; the modes go to the slots
    }
    if (haveChart) { // before any device is opened
        const std::string refusal = batchChartRefusal(chartText, batch < 0 ? 0 : batch, charts);
        if (!refusal.empty()) {
            std::fprintf(stderr, "eqvio_sim: %s\n", refusal.c_str());
            return 2;
        }
    }
    if (batch != 0) { // what the filter batch refuses, before any device is opened
        const char* why = batch < 1 ? "--batch needs B >= 1"
                          : !fs.fastRiccati ? "--batch needs --fastRiccati 1 (the batch has fast Riccati only; the default is 0)"
                          : fs.coordinateChoice == CoordinateChoice::Normal ? "--batch does not support the Normal chart"
                          : sim.maxFeatures > EQF_BATCH_MAX_LANDMARKS ? "--batch holds at most 64 landmarks per run: --maxFeatures <= 64"
                          : fullState ? "--batch does not support --fullState"
                          : landmarkResetTime >= 0 ? "--batch does not support --landmarkReset"
                          : !outputDir.empty() ? "--batch does not support --output"
                          : !datasetDir.empty() ? "--batch does not support --writeDataset"
                          : sigmaFP32 ? "--batch does not support --sigmaFP32"
                          : nullptr;
        if (why) {
            std::fprintf(stderr, "eqvio_sim: %s\n", why);
            return 2;
        }
        if (haveSweep) {
            std::string refusal = sweepRefusal(sweep, batch, batchSettings(fs));
            if (refusal.empty() && haveChart)
                refusal = batchChartSweepRefusal(sweep);
            if (!refusal.empty()) {
                std::fprintf(stderr, "eqvio_sim: %s\n", refusal.c_str());
                return 2;
            }
        }
        return runBatch(sim, fs, batch, quiet, sweep, innovation, recordDir, riccati, charts);
    }
    double lastLandmarkReset = landmarkResetTime > 0 ? 0.0 : std::nan("");

    SimulationDataServer simDataServer(sim, fs);
    loopTimer.initialise({"correction", "features", "preprocessing", "propagation", "total", "total vision update", "write output"});
    // camera extrinsics provided by the data server override the filter settings (main_sim.cpp:97-101)
    fs.cameraOffset = *simDataServer.cameraExtrinsics();
    // the initial condition carries ALL world points (main_sim.cpp:105); the first augmentLandmarkStates trims it
    fs.maxLandmarks = std::max(fs.maxLandmarks, sim.numPoints + (int)sim.maxFeatures);

    std::unique_ptr<VIOWriter> vioWriter; // main_sim.cpp:108-122 (writeState)
    if (!outputDir.empty())
        vioWriter = std::make_unique<VIOWriter>(outputDir);

    // --writeDataset DIR: the measurements of this run in the ASL layout eqvio_opt reads (imu.csv with ns stamps; the
    // feature tracks are features.csv of --output), plus the ground-truth poses
    std::ofstream imuOut, gtOut;
    if (!datasetDir.empty()) {
        if (datasetDir.back() != '/')
            datasetDir += '/';
        VIOWriter makeDir(datasetDir);
        imuOut.open(datasetDir + "imu.csv");
        imuOut << "#timestamp [ns],w_RS_S_x [rad s^-1],w_RS_S_y [rad s^-1],w_RS_S_z [rad s^-1],a_RS_S_x [m s^-2],a_RS_S_y [m s^-2],a_RS_S_z [m s^-2]\n";
        gtOut.open(datasetDir + "groundtruth.csv");
        gtOut << "#timestamp [ns],p_RS_R_x [m],p_RS_R_y [m],p_RS_R_z [m],q_RS_w [],q_RS_x [],q_RS_y [],q_RS_z []\n";
    }

    try {
        VIOFilter filter(simDataServer.getInitialCondition(), fs);
        if (sigmaFP32) // BASELINE config 5: Sigma stored as float in HBM (include/eqf_hip.h)
            eqf_set_option(filter.eqfState().ctx, EQF_OPT_SIGMA_FP32, 2);
        if (nisLine)
            filter.setInnovationStats(true);
        int imuDataCounter = 0, visionDataCounter = 0;
        double neesSum = 0, neesMax = 0, posErr = 0;
        int neesFailures = 0;
        const auto loopStartTime = std::chrono::steady_clock::now();
        if (!quiet)
            std::cout << "NEES:\n";
        while (true) {
            const MeasurementType measType = simDataServer.nextMeasurementType();
            if (measType == MeasurementType::None)
                break;
            if (measType == MeasurementType::Image) {
                loopTimer.startLoop(); // as in main_opt.cpp:180: timing.csv gets one row per vision frame
                VisionMeasurement measData = simDataServer.getSimVision();
                if (!fullState)
                    filter.augmentLandmarkStates(measData.getIds(), simDataServer.getTrueState(measData.stamp, true));
                filter.processVisionData(measData);
                ++visionDataCounter;
                const VIOState estimatedState = filter.stateEstimate();
                const VIOState trueState = simDataServer.getTrueState(filter.getTime());
                double NEES = std::nan("");
                try {
                    NEES = filter.viewEqFState().computeNEES(trueState);
                } catch (const std::exception&) {
                    // Sigma is factorised on the device (Cholesky-type); a Sigma that is positive definite only up to rounding
                    // (cond > 1e13, e.g. the template's 0.003 px measurement noise) is reported as NaN here, the run goes on
                    ++neesFailures;
                }
                if (NEES == NEES) {
                    neesSum += NEES;
                    neesMax = std::max(neesMax, NEES);
                }
                posErr = eqf::norm(estimatedState.sensor.pose.x - trueState.sensor.pose.x);
                if (vioWriter) { // main_sim.cpp:149-154
                    vioWriter->writeStates(filter.getTime(), estimatedState);
                    vioWriter->writeFeatures(measData);
                    vioWriter->writeLandmarkError(filter.getTime(), trueState, estimatedState);
                    vioWriter->writeConsistency(filter.getTime(), trueState, filter.viewEqFState());
                    vioWriter->writeTiming(loopTimer.getLoopTimingData());
                }
                if (!quiet)
                    std::cout << '\r' << NEES << std::flush;
            } else {
                const IMUVelocity imuData = simDataServer.getIMU();
                if (imuOut.is_open()) {
                    imuOut << std::llround(imuData.stamp * 1e9) << std::setprecision(17) << ',' << imuData.gyr.x << ',' << imuData.gyr.y << ',' << imuData.gyr.z << ','
                           << imuData.acc.x << ',' << imuData.acc.y << ',' << imuData.acc.z << '\n';
                    const VIOState t = simDataServer.getTrueState(imuData.stamp);
                    gtOut << std::llround(imuData.stamp * 1e9) << std::setprecision(17) << ',' << t.sensor.pose.x.x << ',' << t.sensor.pose.x.y << ',' << t.sensor.pose.x.z << ','
                          << t.sensor.pose.R.w << ',' << t.sensor.pose.R.x << ',' << t.sensor.pose.R.y << ',' << t.sensor.pose.R.z << '\n';
                }
                filter.processIMUData(imuData);
                ++imuDataCounter;
                if (filter.getTime() >= lastLandmarkReset + landmarkResetTime) { // false while lastLandmarkReset is NaN
                    lastLandmarkReset += landmarkResetTime;
                    filter.setLandmarks(simDataServer.getTrueState(filter.getTime(), true).cameraLandmarks);
                }
            }
        }
        const double elapsed = std::chrono::duration<double>(std::chrono::steady_clock::now() - loopStartTime).count();
        std::cout << "\n\nProcessed " << imuDataCounter << " IMU and " << visionDataCounter << " vision measurements.\n"
                  << "Time taken: " << elapsed << " seconds." << std::endl;
        std::printf("mean NEES %.6g  max NEES %.6g  final position error %.6g m  landmarks %d  vision updates/s %.1f\n", neesSum / std::max(visionDataCounter - neesFailures, 1), neesMax,
                    posErr, filter.viewEqFState().numLandmarks(), visionDataCounter / elapsed);
        if (nisLine) { // the wording of --batch B --innovation's per-run line
            long updates = 0, dof = 0;
            double nis = 0, logdet = 0;
            filter.innovationTotals(updates, dof, nis, logdet);
            std::printf("innovation: updates %ld  mean NIS/dof %.9g  log-likelihood %.9g\n", updates, nis / (double)dof, -0.5 * (nis + logdet + (double)dof * std::log(2.0 * M_PI)));
        }
    } catch (const std::exception& e) {
        std::fprintf(stderr, "eqvio_sim: %s\n", e.what());
        return 1;
    }
    return 0;
}
