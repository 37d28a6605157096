// The functions of klatt_math.h as the host compiles them and as the device compiles them, over caller-given arguments
// (compiled and loaded by tests/test_device_math.py with the engine's own hipcc flags; a second build with
// -DKLATT_NO_SCALAR_CONSTANTS lets the compiler emit its own fused multiply-adds instead of the inline asm).
//   math_host(fn, in, out, n)    the KLATT_HD functions on the host
//   math_device(fn, in, out, n)  the same on device 0: hipMalloc, copy, launch, copy back, free; returns the HIP error
// fn: 0 fast_exp, 1 fast_cos, 2 fast_sin, 3 exp_unreduced, 4 cos_unreduced, 5 cos_quadrant_m1, 6 exp_is_unreduced,
// 7 cos_is_unreduced, 8 cos_is_quadrant_m1 (the predicates return 1.0 or 0.0).
#include <hip/hip_runtime.h>

#include "../../nvspeechplayer_amd/csrc/klatt_math.h"

namespace {

constexpr int kFunctions = 9;

template <int FN>
KLATT_HD double eval(double x)
{
    if (FN == 0) return klatt::fast_exp(x);
    if (FN == 1) return klatt::fast_cos(x);
    if (FN == 2) return klatt::fast_sin(x);
    if (FN == 3) return klatt::exp_unreduced(x);
    if (FN == 4) return klatt::cos_unreduced(x);
    if (FN == 5) return klatt::cos_quadrant_m1(x);
    if (FN == 6) return klatt::exp_is_unreduced(x) ? 1.0 : 0.0;
    if (FN == 7) return klatt::cos_is_unreduced(x) ? 1.0 : 0.0;
    return klatt::cos_is_quadrant_m1(x) ? 1.0 : 0.0;
}

template <int FN>
__global__ void __launch_bounds__(256) probe_kernel(const double* __restrict__ in, double* __restrict__ out, long long n)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) out[i] = eval<FN>(in[i]);
}

template <int FN>
void host_loop(const double* in, double* out, long long n)
{
    for (long long i = 0; i < n; ++i) out[i] = eval<FN>(in[i]);
}

template <int FN>
hipError_t launch(const double* in, double* out, long long n)
{
    const long long blocks = (n + 255) / 256;
    hipLaunchKernelGGL(probe_kernel<FN>, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, 0, in, out, n);
    return hipGetLastError();
}

}  // namespace

extern "C" int math_host(int fn, const double* in, double* out, long long n)
{
    switch (fn) {
    case 0: host_loop<0>(in, out, n); return 0;
    case 1: host_loop<1>(in, out, n); return 0;
    case 2: host_loop<2>(in, out, n); return 0;
    case 3: host_loop<3>(in, out, n); return 0;
    case 4: host_loop<4>(in, out, n); return 0;
    case 5: host_loop<5>(in, out, n); return 0;
    case 6: host_loop<6>(in, out, n); return 0;
    case 7: host_loop<7>(in, out, n); return 0;
    case 8: host_loop<8>(in, out, n); return 0;
    }
    return -1;
}

extern "C" int math_device(int fn, const double* in, double* out, long long n)
{
    if (fn < 0 || fn >= kFunctions || n < 0) return -1;
    if (n == 0) return 0;
    double* d = nullptr;
    const size_t bytes = (size_t)n * sizeof(double);
    hipError_t e = hipMalloc(&d, 2 * bytes);
    if (e != hipSuccess) return (int)e;
    e = hipMemcpy(d, in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        switch (fn) {
        case 0: e = launch<0>(d, d + n, n); break;
        case 1: e = launch<1>(d, d + n, n); break;
        case 2: e = launch<2>(d, d + n, n); break;
        case 3: e = launch<3>(d, d + n, n); break;
        case 4: e = launch<4>(d, d + n, n); break;
        case 5: e = launch<5>(d, d + n, n); break;
        case 6: e = launch<6>(d, d + n, n); break;
        case 7: e = launch<7>(d, d + n, n); break;
        default: e = launch<8>(d, d + n, n); break;
        }
    }
    if (e == hipSuccess) e = hipMemcpy(out, d + n, bytes, hipMemcpyDeviceToHost);
    const hipError_t f = hipFree(d);
    return (int)(e != hipSuccess ? e : f);
}
