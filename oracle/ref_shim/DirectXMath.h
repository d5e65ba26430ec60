// Stand-in for <DirectXMath.h>: the project's own restatement of the DirectXMath functions the reference calls
// (oracle/dxmath_restate.h), made visible under the names the reference's stdafx.h opens with its using-directives.
// Reference and oracle therefore share one DirectXMath; what libref.so pins is everything written on top of it.
#pragma once
#include "dxmath_restate.h"
namespace DirectX {
using namespace ::orc;
namespace PackedVector {
using namespace ::orc;
}
}  // namespace DirectX
