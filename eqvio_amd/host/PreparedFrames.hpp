// eqvio_frames (include/eqvio_filter.h), shared by the replay entry points of filter_capi.cpp and VIOFilterBatch.cpp.
#pragma once
#include "VIOFilter.hpp"
#include "eqvio_filter.h"
#include <vector>

// Prepared replay: the IMU samples and the VisionMeasurement objects (a std::map per frame, as the reference's tracker / data
// server hands them to the filter, main_opt.cpp:196-214) are built once, outside any timed region.
struct eqvio_frames {
    eqvio_amd::GICameraPtr camPtr;
    std::vector<eqvio_amd::VisionMeasurement> meas;
    std::vector<eqvio_amd::IMUVelocity> imus;
    std::vector<size_t> imuBegin; // nframes + 1 offsets into imus
};
