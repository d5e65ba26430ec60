// rt_error.h -- the thread's error text behind rt_last_error(): one string for every translation unit of librt_hip.so
// (defined in rt_scene_prep.cpp, the unit that also builds without HIP).
#pragma once

#include <string>

namespace rtprep {

int Fail(int code, const std::string& msg);  // records msg, returns code
const char* LastError();

}  // namespace rtprep
