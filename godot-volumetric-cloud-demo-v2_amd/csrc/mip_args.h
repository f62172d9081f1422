// mip_args.h -- the one argument rule of the two mip-chain builders, csky_build_mips (assets.cpp, host loops) and csky_build_mips_device
// (api.cpp, mip_level_kernel): what both refuse before they touch `vol`.  Free of HIP, like noise_set.h: tests/mip_args_host builds it with g++ and
// tests/test_bake_reference.py asks it about level counts up to 64.
#pragma once

namespace csky {

// A chain of `levels` levels exists when level levels - 1 still has a texel: n >> (levels - 1) >= 1.  The count is bounded FIRST: a shift of an
// int by 32 or more is undefined, and x86 takes the count modulo 32, which made n = 4, levels = 33 look like levels = 1 to the device entry point
// while chain_offset and the launches behind it ran 33 levels with n >> l wrapped back to n.  With levels <= 31 the shift is at most 30.
// The device form is the stricter one: a power-of-two n <= 1024 and at most 4 channels (the kernels' index arithmetic is sized for that).
inline bool mip_args_ok(const void* vol, int n, int ch, int levels, bool device) {
    if (!vol || n < 1 || ch < 1 || levels < 1 || levels > 31) return false;
    if ((n >> (levels - 1)) < 1) return false;
    if (device && (n > 1024 || (n & (n - 1)) || ch > 4)) return false;
    return true;
}

}  // namespace csky
