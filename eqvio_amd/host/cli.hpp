// Flag parsing shared by the two mains (eqvio_sim, eqvio_opt). The reference reads these values from the "eqf:" block of
// a YAML file (VIOFilterSettings.h:126-174); yaml-cpp is not in this image, so every key is a --flag of the same name.
#pragma once
#include "VIOFilter.hpp"
#include "eqf_batch.h"
#include "eqvio_batch.h"
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

namespace eqvio_amd {

// returns true when `a` was a filter-settings flag (and consumed its value through val())
inline bool parseFilterFlag(const std::string& a, const std::function<const char*()>& val, VIOFilter::Settings& fs) {
    struct D { const char* name; double VIOFilter::Settings::*p; };
    static const D doubles[] = {
        {"--biasOmegaProcessVariance", &VIOFilter::Settings::biasOmegaProcessVariance}, {"--biasAccelProcessVariance", &VIOFilter::Settings::biasAccelProcessVariance},
        {"--attitudeProcessVariance", &VIOFilter::Settings::attitudeProcessVariance}, {"--positionProcessVariance", &VIOFilter::Settings::positionProcessVariance},
        {"--velocityProcessVariance", &VIOFilter::Settings::velocityProcessVariance}, {"--cameraAttitudeProcessVariance", &VIOFilter::Settings::cameraAttitudeProcessVariance},
        {"--cameraPositionProcessVariance", &VIOFilter::Settings::cameraPositionProcessVariance}, {"--pointProcessVariance", &VIOFilter::Settings::pointProcessVariance},
        {"--velGyrNoise", &VIOFilter::Settings::velGyrNoise}, {"--velAccNoise", &VIOFilter::Settings::velAccNoise},
        {"--velGyrBiasWalk", &VIOFilter::Settings::velGyrBiasWalk}, {"--velAccBiasWalk", &VIOFilter::Settings::velAccBiasWalk},
        {"--measurementNoise", &VIOFilter::Settings::measurementNoise}, {"--outlierThresholdAbs", &VIOFilter::Settings::outlierThresholdAbs},
        {"--outlierThresholdProb", &VIOFilter::Settings::outlierThresholdProb}, {"--featureRetention", &VIOFilter::Settings::featureRetention},
        {"--initialAttitudeVariance", &VIOFilter::Settings::initialAttitudeVariance}, {"--initialPositionVariance", &VIOFilter::Settings::initialPositionVariance},
        {"--initialVelocityVariance", &VIOFilter::Settings::initialVelocityVariance}, {"--initialCameraAttitudeVariance", &VIOFilter::Settings::initialCameraAttitudeVariance},
        {"--initialCameraPositionVariance", &VIOFilter::Settings::initialCameraPositionVariance}, {"--initialPointVariance", &VIOFilter::Settings::initialPointVariance},
        {"--initialPointDepthVariance", &VIOFilter::Settings::initialPointDepthVariance}, {"--initialBiasOmegaVariance", &VIOFilter::Settings::initialBiasOmegaVariance},
        {"--initialBiasAccelVariance", &VIOFilter::Settings::initialBiasAccelVariance}, {"--initialSceneDepth", &VIOFilter::Settings::initialSceneDepth},
    };
    struct B { const char* name; bool VIOFilter::Settings::*p; };
    static const B bools[] = {
        {"--useDiscreteInnovationLift", &VIOFilter::Settings::useDiscreteInnovationLift}, {"--useDiscreteVelocityLift", &VIOFilter::Settings::useDiscreteVelocityLift},
        {"--useDiscreteStateMatrix", &VIOFilter::Settings::useDiscreteStateMatrix}, {"--fastRiccati", &VIOFilter::Settings::fastRiccati},
        {"--useMedianDepth", &VIOFilter::Settings::useMedianDepth}, {"--useEquivariantOutput", &VIOFilter::Settings::useEquivariantOutput},
        {"--removeLostLandmarks", &VIOFilter::Settings::removeLostLandmarks},
    };
    for (const D& d : doubles)
        if (a == d.name) {
            fs.*(d.p) = std::atof(val());
            return true;
        }
    for (const B& b : bools)
        if (a == b.name) {
            fs.*(b.p) = std::atoi(val()) != 0;
            return true;
        }
    if (a == "--coordinateChoice") { // coordinateSelection, VIOFilterSettings.h:33-46
        const std::string c = val();
        if (c == "Euclidean")
            fs.coordinateChoice = CoordinateChoice::Euclidean;
        else if (c == "InvDepth")
            fs.coordinateChoice = CoordinateChoice::InvDepth;
        else
            throw std::runtime_error("Invalid coordinate choice. Valid choices on the MI355X path are Euclidean, InvDepth.");
        return true;
    }
    if (a == "--device") {
        fs.device = std::atoi(val());
        return true;
    }
    if (a == "--maxLandmarks") {
        fs.maxLandmarks = std::atoi(val());
        return true;
    }
    return false;
}

// ---- what the two mains share of --batch B --sweep NAME=v0,...: the settings as the C-ABI's struct, one of its fields by name, the refusals

// --sweep NAME=v0,v1,...: one field of eqvio_settings by its name, one value per slot
struct Sweep {
    std::string name;
    std::vector<std::string> values;
};
// the argument of --sweep: NAME=v0,v1,... (no '=': a name without values, which sweepRefusal refuses)
inline Sweep parseSweep(const std::string& v) {
    Sweep sweep;
    const size_t eq = v.find('=');
    sweep.name = v.substr(0, eq);
    for (size_t p = eq == std::string::npos ? v.size() : eq + 1; p <= v.size() && eq != std::string::npos;) {
        const size_t c = std::min(v.find(',', p), v.size());
        sweep.values.push_back(v.substr(p, c - p));
        p = c + 1;
    }
    return sweep;
}
inline bool setSettingsField(eqvio_settings& es, const std::string& name, const std::string& value, std::string& why) {
    struct D { const char* name; double eqvio_settings::*p; };
    static const D doubles[] = {
        {"biasOmegaProcessVariance", &eqvio_settings::biasOmegaProcessVariance}, {"biasAccelProcessVariance", &eqvio_settings::biasAccelProcessVariance},
        {"attitudeProcessVariance", &eqvio_settings::attitudeProcessVariance}, {"positionProcessVariance", &eqvio_settings::positionProcessVariance},
        {"velocityProcessVariance", &eqvio_settings::velocityProcessVariance}, {"cameraAttitudeProcessVariance", &eqvio_settings::cameraAttitudeProcessVariance},
        {"cameraPositionProcessVariance", &eqvio_settings::cameraPositionProcessVariance}, {"pointProcessVariance", &eqvio_settings::pointProcessVariance},
        {"velGyrNoise", &eqvio_settings::velGyrNoise}, {"velAccNoise", &eqvio_settings::velAccNoise},
        {"velGyrBiasWalk", &eqvio_settings::velGyrBiasWalk}, {"velAccBiasWalk", &eqvio_settings::velAccBiasWalk},
        {"measurementNoise", &eqvio_settings::measurementNoise}, {"outlierThresholdAbs", &eqvio_settings::outlierThresholdAbs},
        {"outlierThresholdProb", &eqvio_settings::outlierThresholdProb}, {"featureRetention", &eqvio_settings::featureRetention},
        {"initialAttitudeVariance", &eqvio_settings::initialAttitudeVariance}, {"initialPositionVariance", &eqvio_settings::initialPositionVariance},
        {"initialVelocityVariance", &eqvio_settings::initialVelocityVariance}, {"initialCameraAttitudeVariance", &eqvio_settings::initialCameraAttitudeVariance},
        {"initialCameraPositionVariance", &eqvio_settings::initialCameraPositionVariance}, {"initialPointVariance", &eqvio_settings::initialPointVariance},
        {"initialPointDepthVariance", &eqvio_settings::initialPointDepthVariance}, {"initialBiasOmegaVariance", &eqvio_settings::initialBiasOmegaVariance},
        {"initialBiasAccelVariance", &eqvio_settings::initialBiasAccelVariance}, {"initialSceneDepth", &eqvio_settings::initialSceneDepth},
    };
    struct I { const char* name; int eqvio_settings::*p; };
    static const I ints[] = {
        {"useDiscreteInnovationLift", &eqvio_settings::useDiscreteInnovationLift}, {"useDiscreteVelocityLift", &eqvio_settings::useDiscreteVelocityLift},
        {"useDiscreteStateMatrix", &eqvio_settings::useDiscreteStateMatrix}, {"fastRiccati", &eqvio_settings::fastRiccati},
        {"useMedianDepth", &eqvio_settings::useMedianDepth}, {"useFeaturePredictions", &eqvio_settings::useFeaturePredictions},
        {"useEquivariantOutput", &eqvio_settings::useEquivariantOutput}, {"removeLostLandmarks", &eqvio_settings::removeLostLandmarks},
    };
    char* end = nullptr;
    for (const D& d : doubles)
        if (name == d.name) {
            es.*(d.p) = std::strtod(value.c_str(), &end);
            if (value.empty() || *end)
                why = "--sweep " + name + ": '" + value + "' is not a number";
            return true;
        }
    for (const I& i : ints)
        if (name == i.name) {
            es.*(i.p) = (int)std::strtol(value.c_str(), &end, 10);
            if (value.empty() || *end)
                why = "--sweep " + name + ": '" + value + "' is not an integer";
            return true;
        }
    if (name == "coordinateChoice") { // by name, or the enum's number; which charts the batch takes is eqf_batch_check_settings's to say
        const char* charts[3] = {"Euclidean", "InvDepth", "Normal"};
        const int enums[3] = {EQVIO_COORD_EUCLIDEAN, EQVIO_COORD_INVDEPTH, EQVIO_COORD_NORMAL};
        const size_t c = std::find(charts, charts + 3, value) - charts;
        es.coordinateChoice = c < 3 ? enums[c] : (int)std::strtol(value.c_str(), &end, 10);
        if (c == 3 && (value.empty() || *end))
            why = "--sweep coordinateChoice: '" + value + "' is neither Euclidean, InvDepth nor a number";
        return true;
    }
    return false;
}
// what --sweep is refused for, before any device is opened (empty: nothing). es: the settings of the run without the swept field. Whether the batch takes
// slot k's settings is asked of the batch (eqf_batch_check_settings), not restated here.
inline std::string sweepRefusal(const Sweep& sw, int B, const eqvio_settings& es) {
    if (sw.name.empty() || sw.values.empty())
        return "--sweep needs NAME=v0,v1,...";
    for (const std::string& v : sw.values) {
        eqvio_settings ek = es;
        std::string why;
        if (!setSettingsField(ek, sw.name, v, why))
            return "--sweep: '" + sw.name + "' is not a field of eqvio_settings";
        if (!why.empty())
            return why;
        if (const int rc = eqf_batch_check_settings(&ek))
            return "--sweep " + sw.name + "=" + v + ": the batch refuses these settings (" + eqf_error_string(rc) + ")";
    }
    if ((int)sw.values.size() != B)
        return "--sweep has " + std::to_string(sw.values.size()) + " values for --batch " + std::to_string(B) + ": one value per slot";
    return "";
}
// what a sweep is refused for behind a warm-up (--warmup F, F > 0), where the value reaches a filter that already runs: the chart cannot change under a slot
// that holds landmarks (eqf_batch_set_slot_settings), and the initial variances of the sensor state are read only when a filter starts, so every slot would
// score the same. initialPointVariance, initialPointDepthVariance and initialSceneDepth are read for every new landmark and stay.
inline std::string warmupSweepRefusal(const Sweep& sw) {
    static const char* const atStart[] = {"initialAttitudeVariance", "initialPositionVariance", "initialVelocityVariance", "initialCameraAttitudeVariance",
                                          "initialCameraPositionVariance", "initialBiasOmegaVariance", "initialBiasAccelVariance"};
    if (sw.name == "coordinateChoice")
        return "--warmup with --sweep coordinateChoice: the chart cannot change under a filter that holds landmarks";
    for (const char* n : atStart)
        if (sw.name == n)
            return "--warmup with --sweep " + sw.name + ": it is read only when a filter starts, so it has no effect behind a warm-up";
    return "";
}

// --batchRiccati M[,M...] with --batch B: the slots' propagation (eqvio_batch_set_slot_riccati, _set_slot_state_matrix), M = fast | accurate | discrete -
// discrete is the accurate mode with the discrete state matrix, BATCH_CLI_DISCRETE in `modes` -; one value for every slot, or B values, one per slot. Returns what the flag is refused for, before any file or device is opened (empty: nothing); modes then holds B entries.
constexpr int BATCH_CLI_DISCRETE = 2; // the flag's third word: EQVIO_BATCH_RICCATI_ACCURATE with EQVIO_BATCH_STATE_MATRIX_DISCRETE
inline std::string batchRiccatiRefusal(const std::string& text, int B, std::vector<int>& modes) {
    if (B == 0)
        return "--batchRiccati needs --batch B (the mode is the filter batch's, per slot)";
    std::vector<int> given;
    for (size_t p = 0; p <= text.size();) {
        const size_t c = std::min(text.find(',', p), text.size());
        const std::string w = text.substr(p, c - p);
        if (w != "fast" && w != "accurate" && w != "discrete")
            return "--batchRiccati: '" + w + "' is neither fast nor accurate nor discrete";
        given.push_back(w == "discrete" ? BATCH_CLI_DISCRETE : w == "accurate" ? EQVIO_BATCH_RICCATI_ACCURATE : EQVIO_BATCH_RICCATI_FAST);
        p = c + 1;
    }
    if (given.size() != 1 && (int)given.size() != B)
        return "--batchRiccati has " + std::to_string(given.size()) + " values for --batch " + std::to_string(B) + ": one value, or one per slot";
    modes.assign(std::max(B, 0), given[0]);
    for (int k = 0; k < B && given.size() > 1; ++k)
        modes[k] = given[k];
    return "";
}
inline const char* batchRiccatiName(int mode) { return mode == BATCH_CLI_DISCRETE ? "discrete" : mode == EQVIO_BATCH_RICCATI_ACCURATE ? "accurate" : "fast"; }
// the two per-slot choices one word of the flag stands for
inline int batchCliRiccati(int mode) { return mode == EQVIO_BATCH_RICCATI_FAST ? EQVIO_BATCH_RICCATI_FAST : EQVIO_BATCH_RICCATI_ACCURATE; }
inline int batchCliStateMatrix(int mode) { return mode == BATCH_CLI_DISCRETE ? EQVIO_BATCH_STATE_MATRIX_DISCRETE : EQVIO_BATCH_STATE_MATRIX_CONTINUOUS; }

// --batchChart C[,C...] with --batch B: the slots' coordinate chart (eqvio_batch_set_slot_chart), C = euclidean | invdepth | normal; one value for every slot, or
// B values, one per slot. The one way to the Normal chart in a batch: --coordinateChoice Normal and --sweep coordinateChoice=...,Normal stay refused, as the
// settings calls refuse it. Returns what the flag is refused for, before any file or device is opened (empty: nothing); charts then holds B entries.
inline std::string batchChartRefusal(const std::string& text, int B, std::vector<int>& charts) {
    if (B == 0)
        return "--batchChart needs --batch B (the chart is the filter batch's, per slot)";
    std::vector<int> given;
    for (size_t p = 0; p <= text.size();) {
        const size_t c = std::min(text.find(',', p), text.size());
        const std::string w = text.substr(p, c - p);
        if (w != "euclidean" && w != "invdepth" && w != "normal")
            return "--batchChart: '" + w + "' is neither euclidean nor invdepth nor normal";
        given.push_back(w == "normal" ? EQVIO_COORD_NORMAL : w == "invdepth" ? EQVIO_COORD_INVDEPTH : EQVIO_COORD_EUCLIDEAN);
        p = c + 1;
    }
    if (given.size() != 1 && (int)given.size() != B)
        return "--batchChart has " + std::to_string(given.size()) + " values for --batch " + std::to_string(B) + ": one value, or one per slot";
    charts.assign(std::max(B, 0), given[0]);
    for (int k = 0; k < B && given.size() > 1; ++k)
        charts[k] = given[k];
    return "";
}
// --batchChart beside a sweep of the chart itself: two flags would name the slots' charts, and the later call would silently win
inline std::string batchChartSweepRefusal(const Sweep& sw) {
    return sw.name == "coordinateChoice" ? "--batchChart with --sweep coordinateChoice: both name the slots' charts; give one of them" : "";
}
// --rechart C[,C...] with --batch B --warmup F: slot k is converted to chart C_k at the branch (eqvio_batch_convert_chart), C = euclidean | invdepth | normal; one
// value for every slot, or B values, one per slot. What the flag is refused for on its own words and beside the other chart flags, before any file or device is
// opened (empty: nothing); charts then holds B entries. That it needs a warm-up is rechartWarmupRefusal's to say, once --warmup has been read.
inline std::string rechartRefusal(const std::string& text, int B, bool haveBatchChart, const Sweep& sw, std::vector<int>& charts) {
    if (B == 0)
        return "--rechart needs --batch B (the slots branch into the charts)";
    std::vector<int> given;
    for (size_t p = 0; p <= text.size();) {
        const size_t c = std::min(text.find(',', p), text.size());
        const std::string w = text.substr(p, c - p);
        if (w != "euclidean" && w != "invdepth" && w != "normal")
            return "--rechart: '" + w + "' is neither euclidean nor invdepth nor normal";
        given.push_back(w == "normal" ? EQVIO_COORD_NORMAL : w == "invdepth" ? EQVIO_COORD_INVDEPTH : EQVIO_COORD_EUCLIDEAN);
        p = c + 1;
    }
    if (given.size() != 1 && (int)given.size() != B)
        return "--rechart has " + std::to_string(given.size()) + " values for --batch " + std::to_string(B) + ": one value, or one per slot";
    if (haveBatchChart)
        return "--rechart with --batchChart: --batchChart names the charts the slots start in, and a warm-up runs under the settings' chart; give one of them";
    if (sw.name == "coordinateChoice")
        return "--rechart with --sweep coordinateChoice: both name the slots' charts; give one of them";
    charts.assign(std::max(B, 0), given[0]);
    for (int k = 0; k < B && given.size() > 1; ++k)
        charts[k] = given[k];
    return "";
}
inline std::string rechartWarmupRefusal(int warmup) {
    return warmup > 0 ? "" : "--rechart needs --warmup F with F > 0 (the slots are converted where they branch from the warm-up)";
}
inline const char* batchChartName(int chart) { return chart == EQVIO_COORD_NORMAL ? "normal" : chart == EQVIO_COORD_INVDEPTH ? "invdepth" : "euclidean"; }
// --branchAt F --branchCharts C[,C...] on the single-filter path: F vision frames on one filter, which is then copied into one fresh filter per chart
// (VIOFilter::copyFrom), each copy converted (VIOFilter::convertChart); every branch runs the remaining frames. What the pair is refused for, the flag named,
// before any file or device is opened (empty: nothing); frames and charts are then set.
inline std::string branchRefusal(bool haveAt, const std::string& atText, bool haveCharts, const std::string& chartsText, int batch, int& frames, std::vector<int>& charts) {
    if (batch != 0)
        return std::string(haveAt ? "--branchAt" : "--branchCharts") + " is the single filter's branch; with --batch B the slots branch by --warmup F --rechart C,...";
    if (!haveCharts)
        return "--branchAt needs --branchCharts C[,C...] (the charts the filter branches into)";
    if (!haveAt)
        return "--branchCharts needs --branchAt F (the vision frame the filter branches at)";
    char* end = nullptr;
    const long f = std::strtol(atText.c_str(), &end, 10);
    if (atText.empty() || *end)
        return "--branchAt: '" + atText + "' is not a number of frames";
    if (f <= 0 || f > 1000000000)
        return "--branchAt " + atText + ": needs 0 < F, and no more frames than a sequence has";
    charts.clear();
    for (size_t p = 0; p <= chartsText.size();) {
        const size_t c = std::min(chartsText.find(',', p), chartsText.size());
        const std::string w = chartsText.substr(p, c - p);
        if (w != "euclidean" && w != "invdepth" && w != "normal")
            return "--branchCharts: '" + w + "' is neither euclidean nor invdepth nor normal";
        charts.push_back(w == "normal" ? EQVIO_COORD_NORMAL : w == "invdepth" ? EQVIO_COORD_INVDEPTH : EQVIO_COORD_EUCLIDEAN);
        p = c + 1;
    }
    frames = (int)f;
    return "";
}

// the filter settings as the C-ABI's eqvio_settings
inline eqvio_settings batchSettings(const VIOFilter::Settings& fs) {
    eqvio_settings es;
    std::memset(&es, 0, sizeof(es));
    es.biasOmegaProcessVariance = fs.biasOmegaProcessVariance, es.biasAccelProcessVariance = fs.biasAccelProcessVariance;
    es.attitudeProcessVariance = fs.attitudeProcessVariance, es.positionProcessVariance = fs.positionProcessVariance;
    es.velocityProcessVariance = fs.velocityProcessVariance, es.cameraAttitudeProcessVariance = fs.cameraAttitudeProcessVariance;
    es.cameraPositionProcessVariance = fs.cameraPositionProcessVariance, es.pointProcessVariance = fs.pointProcessVariance;
    es.velGyrNoise = fs.velGyrNoise, es.velAccNoise = fs.velAccNoise, es.velGyrBiasWalk = fs.velGyrBiasWalk, es.velAccBiasWalk = fs.velAccBiasWalk;
    es.measurementNoise = fs.measurementNoise, es.outlierThresholdAbs = fs.outlierThresholdAbs, es.outlierThresholdProb = fs.outlierThresholdProb;
    es.featureRetention = fs.featureRetention;
    es.initialAttitudeVariance = fs.initialAttitudeVariance, es.initialPositionVariance = fs.initialPositionVariance;
    es.initialVelocityVariance = fs.initialVelocityVariance, es.initialCameraAttitudeVariance = fs.initialCameraAttitudeVariance;
    es.initialCameraPositionVariance = fs.initialCameraPositionVariance, es.initialPointVariance = fs.initialPointVariance;
    es.initialPointDepthVariance = fs.initialPointDepthVariance, es.initialBiasOmegaVariance = fs.initialBiasOmegaVariance;
    es.initialBiasAccelVariance = fs.initialBiasAccelVariance, es.initialSceneDepth = fs.initialSceneDepth;
    es.useDiscreteInnovationLift = fs.useDiscreteInnovationLift, es.useDiscreteVelocityLift = fs.useDiscreteVelocityLift;
    es.useDiscreteStateMatrix = fs.useDiscreteStateMatrix, es.fastRiccati = fs.fastRiccati, es.useMedianDepth = fs.useMedianDepth;
    es.useFeaturePredictions = fs.useFeaturePredictions, es.useEquivariantOutput = fs.useEquivariantOutput, es.removeLostLandmarks = fs.removeLostLandmarks;
    es.coordinateChoice = (int)fs.coordinateChoice;
    const double offset[7] = {fs.cameraOffset.R.w, fs.cameraOffset.R.x, fs.cameraOffset.R.y, fs.cameraOffset.R.z, fs.cameraOffset.x.x, fs.cameraOffset.x.y, fs.cameraOffset.x.z};
    std::memcpy(es.cameraOffset, offset, sizeof(offset));
    return es;
}

} // namespace eqvio_amd
