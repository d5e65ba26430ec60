// Stand-in for <windows.h>: the reference's headers need only MSVC's __declspec(align(16)) spelling to disappear (the
// types it decorates hold XMVECTORs, which dxmath_restate.h already aligns to 16 bytes).  <functional> is what MSVC's
// standard headers pull in on their own and light.h relies on (std::function).
#pragma once
#include <functional>
#define __declspec(x)
