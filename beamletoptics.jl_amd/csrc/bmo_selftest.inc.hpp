// bmo_selftest.inc.hpp — the engine's checks of its own arithmetic (included by bmo_engine.hip at file scope, behind the pools):
//   selftest_minmax_kernel, selftest_jl_kernel, jl_six   the device side
//   bmo_jl_trig                                          the host build of bmo_jlmath.hpp, one function at a time
//   bmo_selftest                                         device min/max forms against their rules, device libm against the host build
namespace {

// bmo_selftest: the branch-free forms of bmo_lane.hpp against the rules they stand for, bitwise
__global__ void selftest_minmax_kernel(const double* __restrict__ v, int n, int32_t* __restrict__ bad) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i >= n * n) return;
    const double x = v[i / n], y = v[i % n];
    auto same = [](double a, double b) { return (isnan_(a) && isnan_(b)) || __double_as_longlong(a) == __double_as_longlong(b); };
    int form = 0;
    if (!same(jmax(x, y), jmax_rule(x, y))) form = 1;
    else if (!same(jmin(x, y), jmin_rule(x, y))) form = 2;
    else {
        // Dual forms: the winner's value and partials
        const Dual X{x, {1.0, 2.0, 3.0}}, Y{y, {5.0, 6.0, 7.0}};
        const Dual mx = jmax(X, Y), mn = jmin(X, Y), mx0 = jmax(X, y), mn0 = jmin(X, y);
        // (selection, ties and unordered operands to the second argument: bmo_lane.hpp above jsqrt(DualN))
        const bool xwx = x > y, xwn = x < y;
        if (!same(mx.v, xwx ? x : y) || mx.p[0] != (xwx ? 1.0 : 5.0) || mx.p[2] != (xwx ? 3.0 : 7.0)) form = 3;
        else if (!same(mn.v, xwn ? x : y) || mn.p[0] != (xwn ? 1.0 : 5.0) || mn.p[2] != (xwn ? 3.0 : 7.0)) form = 4;
        else if (!same(mx0.v, xwx ? x : y) || mx0.p[1] != (xwx ? 2.0 : 0.0)) form = 5;
        else if (!same(mn0.v, xwn ? x : y) || mn0.p[1] != (xwn ? 2.0 : 0.0)) form = 6;
        const Dual ab = jabs(X);
        if (!form && (!same(ab.v, fabs(x)) || ab.p[0] != (sgn(x) ? -1.0 : 1.0))) form = 7;
    }
    if (form && atomicCAS(bad, -1, i) == -1) bad[1] = form;
}

// Julia Base's elementary functions (bmo_jlmath.hpp) on the device, six results per argument: sin, cos, tan, acos(clamped), atan, atan(1, x)
__host__ __device__ inline void jl_six(double x, double* o) {
    o[0] = jl::sin(x);
    o[1] = jl::cos(x);
    o[2] = jl::tan(x);
    o[3] = jl::acos(x < -1.0 ? -1.0 : (x > 1.0 ? 1.0 : x));
    o[4] = jl::atan(x);
    o[5] = jl::atan2(1.0, x);
}
__global__ void selftest_jl_kernel(const double* __restrict__ x, int n, double* __restrict__ out) {
    const int i = (int)(blockIdx.x * blockDim.x + threadIdx.x);
    if (i < n) jl_six(x[i], out + (size_t)6 * i);
}

}  // namespace

extern "C" {

double bmo_jl_trig(int32_t which, double x, double y) {
    switch (which) {
        case 0: return jl::sin(x);
        case 1: return jl::cos(x);
        case 2: return jl::tan(x);
        case 3: return jl::acos(x);
        case 4: return jl::atan(x);
        case 5: return jl::atan2(y, x);
    }
    return (double)NAN;
}

int bmo_selftest(int32_t device) {
    if (hipSetDevice(device) != hipSuccess) return fail(BMO_ERR_NO_DEVICE, "hipSetDevice");
    const double tiny = 4.9406564584124654e-324, big = 1.7976931348623157e308;
    std::vector<double> v{0.0, -0.0, tiny, -tiny, 2.2250738585072014e-308, -2.2250738585072014e-308, 1.0, -1.0, 1.0000000000000002, 0.5, -0.5, 3.0, -3.0,
                          big, -big, (double)INFINITY, -(double)INFINITY, (double)NAN, -(double)NAN, 1e-10, -1e-10, 1e-300, 123.456, -123.456};
    const int n = (int)v.size();
    DevBuf d_v, d_bad;
    int rc;
    if ((rc = d_v.alloc((size_t)n * 8)) || (rc = d_bad.alloc(16))) return rc;
    HIP_TRY(hipMemcpy(d_v.p, v.data(), (size_t)n * 8, hipMemcpyHostToDevice));
    HIP_TRY(hipMemset(d_bad.p, 0xFF, 16));
    hipLaunchKernelGGL(selftest_minmax_kernel, dim3((unsigned)((n * n + 255) / 256)), dim3(256), 0, 0, (const double*)d_v.p, n, (int32_t*)d_bad.p);
    HIP_TRY(hipGetLastError());
    int32_t bad[4];
    HIP_TRY(hipMemcpy(bad, d_bad.p, 16, hipMemcpyDeviceToHost));
    if (bad[0] != -1)
        return fail(BMO_ERR_INTERNAL, "device min/max differs from the rule: form " + std::to_string(bad[1]) + " on (" + std::to_string(v[(size_t)(bad[0] / n)]) + ", " +
                                          std::to_string(v[(size_t)(bad[0] % n)]) + ")");
    // ... and the elementary functions (bmo_jlmath.hpp): the device's results against this library's host build of the same header, bit for bit
    {
        std::vector<double> xs;
        unsigned long long s = 0x243F6A8885A308D3ull;
        auto rnd = [&]() {
            s = s * 6364136223846793005ull + 1442695040888963407ull;
            return (double)(s >> 11) * 0x1p-53;
        };
        for (int q = 0; q < 4096; ++q) xs.push_back(-7.0 + 14.0 * rnd());            // the reductions by 0 .. 4 pi/2
        for (int q = 0; q < 2048; ++q) xs.push_back(-1.0 + 2.0 * rnd());             // acos's three ranges, the kernels without reduction
        for (int q = 0; q < 1024; ++q) xs.push_back((rnd() < 0.5 ? -1.0 : 1.0) * std::ldexp(1.0 + rnd(), (int)(rnd() * 80) - 40));  // atan's five ranges, tiny and large
        for (int q = 1; q <= 8; ++q)                                                 // next to multiples of pi/2: the three-constant reduction
            for (int e = -3; e <= 3; ++e) xs.push_back(std::nextafter(q * 1.5707963267948966, e < 0 ? -100.0 : 100.0) + e * 1e-9);
        for (double sp : {0.0, -0.0, 1.0, -1.0, 0.5, -0.5, 0.6744, 0.67434, 0.4375, 0.6875, 1.1875, 2.4375, 1e-9, 1e-300, 1e6, 1.5e6, (double)INFINITY, (double)NAN})
            xs.push_back(sp);
        const int m = (int)xs.size();
        DevBuf d_x, d_o;
        if ((rc = d_x.alloc((size_t)m * 8)) || (rc = d_o.alloc((size_t)m * 48))) return rc;
        HIP_TRY(hipMemcpy(d_x.p, xs.data(), (size_t)m * 8, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(selftest_jl_kernel, dim3((unsigned)((m + 255) / 256)), dim3(256), 0, 0, (const double*)d_x.p, m, (double*)d_o.p);
        HIP_TRY(hipGetLastError());
        std::vector<double> got((size_t)m * 6);
        HIP_TRY(hipMemcpy(got.data(), d_o.p, (size_t)m * 48, hipMemcpyDeviceToHost));
        static const char* const names[6] = {"sin", "cos", "tan", "acos", "atan", "atan(1, x)"};
        for (int i = 0; i < m; ++i) {
            double want[6];
            jl_six(xs[(size_t)i], want);
            for (int f = 0; f < 6; ++f) {
                const double a = got[(size_t)6 * i + f], b = want[f];
                if (!((a != a && b != b) || std::memcmp(&a, &b, 8) == 0)) {
                    char buf[160];
                    std::snprintf(buf, sizeof buf, "device %s(%.17g) = %.17g, host build of the same code %.17g", names[f], xs[(size_t)i], a, b);
                    return fail(BMO_ERR_INTERNAL, buf);
                }
            }
        }
    }
    return BMO_OK;
}

}  // extern "C"
