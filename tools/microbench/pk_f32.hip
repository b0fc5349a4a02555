// Microbenchmark: what does a packed fp32 multiply cost in a VALU-only stream at five waves per SIMD, against the two plain multiplies
// it replaces and against itself with the register copies that feed an aligned pair?  (profiles/r08_fp32_pairing.md)
//   mode 0: 16 x v_mul_f32                          per block of the loop body (16 multiplies)
//   mode 1:  8 x v_pk_mul_f32                       (16 multiplies)
//   mode 2:  8 x (v_mov_b32 + v_pk_mul_f32)         (16 multiplies, one copy into the pair per packed op; + 1 to fill the pair)
//   mode 3:  8 x (2 v_mov_b32 + v_pk_mul_f32)       (16 multiplies, both halves of the pair copied)
//   mode 4: 16 x v_mov_b32                          (the copy alone)
// Every stream keeps 16 independent accumulators, multiplies by a lane-varying factor of 1.0 (nothing the compiler or the hardware can
// fold), and is written as inline assembly so that what is timed is exactly the stream named above.  Launch shape of the flagship kernels:
// 256 threads, __launch_bounds__(256, 5), five workgroups per CU resident (grid = CUs x 5).  Standalone: hipcc -O3 --offload-arch=gfx950
// -o build/microbench/pk_f32 tools/microbench/pk_f32.hip; prints ms per launch (event time: the figure to compare) and the median wave's own time per
// block, which shows whether the workgroups were resident together (on the record's runs they were not for the whole launch; the stream is bound by issue slots either way).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

typedef float f2 __attribute__((ext_vector_type(2)));

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)

template <int MODE>
__global__ void __launch_bounds__(256, 5) k_stream(float* __restrict__ out, const float* __restrict__ in, int iters, unsigned long long* __restrict__ cycles)
{
    const uint32_t tid = blockIdx.x * 256u + threadIdx.x;
    const float one = in[tid & 255u];   // 1.0f, but only the host knows
    f2 a0 = {one, one}, a1 = a0, a2 = a0, a3 = a0, a4 = a0, a5 = a0, a6 = a0, a7 = a0, c = {one, one};
    const unsigned long long t0 = wall_clock64();
    for (int i = 0; i < iters; ++i)
    {
        if (MODE == 0)
            asm volatile("v_mul_f32 %0, %0, %16\n v_mul_f32 %1, %1, %17\n v_mul_f32 %2, %2, %16\n v_mul_f32 %3, %3, %17\n"
                         "v_mul_f32 %4, %4, %16\n v_mul_f32 %5, %5, %17\n v_mul_f32 %6, %6, %16\n v_mul_f32 %7, %7, %17\n"
                         "v_mul_f32 %8, %8, %16\n v_mul_f32 %9, %9, %17\n v_mul_f32 %10, %10, %16\n v_mul_f32 %11, %11, %17\n"
                         "v_mul_f32 %12, %12, %16\n v_mul_f32 %13, %13, %17\n v_mul_f32 %14, %14, %16\n v_mul_f32 %15, %15, %17\n"
                         : "+v"(a0.x), "+v"(a0.y), "+v"(a1.x), "+v"(a1.y), "+v"(a2.x), "+v"(a2.y), "+v"(a3.x), "+v"(a3.y),
                           "+v"(a4.x), "+v"(a4.y), "+v"(a5.x), "+v"(a5.y), "+v"(a6.x), "+v"(a6.y), "+v"(a7.x), "+v"(a7.y)
                         : "v"(c.x), "v"(c.y));
        else if (MODE == 1)
            asm volatile("v_pk_mul_f32 %0, %0, %8\n v_pk_mul_f32 %1, %1, %8\n v_pk_mul_f32 %2, %2, %8\n v_pk_mul_f32 %3, %3, %8\n"
                         "v_pk_mul_f32 %4, %4, %8\n v_pk_mul_f32 %5, %5, %8\n v_pk_mul_f32 %6, %6, %8\n v_pk_mul_f32 %7, %7, %8\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c));
        else if (MODE == 2)   // the pair v[40:41] is the copy target (both halves written before the first use: i = 0, 1)
            asm volatile(
                         "v_mov_b32 v41, %9\n"
                         "v_mov_b32 v40, %8  \n v_pk_mul_f32 %0, %0, v[40:41]\n"
                         "v_mov_b32 v41, %9  \n v_pk_mul_f32 %1, %1, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_pk_mul_f32 %2, %2, v[40:41]\n"
                         "v_mov_b32 v41, %9  \n v_pk_mul_f32 %3, %3, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_pk_mul_f32 %4, %4, v[40:41]\n"
                         "v_mov_b32 v41, %9  \n v_pk_mul_f32 %5, %5, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_pk_mul_f32 %6, %6, v[40:41]\n"
                         "v_mov_b32 v41, %9  \n v_pk_mul_f32 %7, %7, v[40:41]\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c.x), "v"(c.y) : "v40", "v41");
        else if (MODE == 3)
            asm volatile(
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %0, %0, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %1, %1, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %2, %2, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %3, %3, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %4, %4, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %5, %5, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %6, %6, v[40:41]\n"
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9  \n v_pk_mul_f32 %7, %7, v[40:41]\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c.x), "v"(c.y) : "v40", "v41");
        else
            asm volatile(
                         "v_mov_b32 v40, %8  \n v_mov_b32 v41, %9\n"
                         "v_mov_b32 v42, %8  \n v_mov_b32 v43, %9\n"
                         "v_mov_b32 v44, %8  \n v_mov_b32 v45, %9\n"
                         "v_mov_b32 v46, %8  \n v_mov_b32 v47, %9\n"
                         "v_mov_b32 v48, %8  \n v_mov_b32 v49, %9\n"
                         "v_mov_b32 v50, %8  \n v_mov_b32 v51, %9\n"
                         "v_mov_b32 v52, %8  \n v_mov_b32 v53, %9\n"
                         "v_mov_b32 v54, %8  \n v_mov_b32 v55, %9\n"
                         : "+v"(a0), "+v"(a1), "+v"(a2), "+v"(a3), "+v"(a4), "+v"(a5), "+v"(a6), "+v"(a7) : "v"(c.x), "v"(c.y) : "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", "v55");
    }
    const unsigned long long t1 = wall_clock64();
    const f2 s = a0 + a1 + a2 + a3 + a4 + a5 + a6 + a7;
    out[tid] = s.x + s.y;
    if (threadIdx.x == 0) cycles[blockIdx.x] = t1 - t0;
}

// dynamic LDS per workgroup, never touched: five workgroups (= five waves per SIMD) fit a CU's 160 KB and no more
constexpr size_t kLdsBallast = 28 * 1024;

template <int MODE>
static int run(const char* name, int vops, int blocks, int iters, float* out, const float* in, unsigned long long* cyc, int clock_khz)
{
    hipEvent_t e0, e1;
    CHECK(hipEventCreate(&e0)); CHECK(hipEventCreate(&e1));
    std::vector<float> ms;
    for (int rep = 0; rep < 6; ++rep)
    {
        CHECK(hipEventRecord(e0));
        hipLaunchKernelGGL(k_stream<MODE>, dim3(blocks), dim3(256), kLdsBallast, 0, out, in, iters, cyc);
        CHECK(hipEventRecord(e1)); CHECK(hipEventSynchronize(e1));
        float t; CHECK(hipEventElapsedTime(&t, e0, e1));
        if (rep) ms.push_back(t);   // first launch loads the code object
    }
    std::sort(ms.begin(), ms.end());
    std::vector<unsigned long long> h(blocks);
    CHECK(hipMemcpy(h.data(), cyc, blocks * sizeof(unsigned long long), hipMemcpyDeviceToHost));
    std::sort(h.begin(), h.end());
    // wall_clock64 counts at a constant rate (hipDeviceAttributeWallClockRate): the median wave's time in ns per block of 16 multiplies;
    // the five waves of a SIMD share its issue port, so the SIMD spends (wave ns / 5) per block and wave
    const double wave_ns = (double)h[blocks / 2] * (1e6 / clock_khz) / iters;
    printf("| %d | %s | %d | %.3f | %.3f | %.2f | %.2f |\n", MODE, name, vops, ms[ms.size() / 2], ms[0], wave_ns / 5.0, wave_ns / 5.0 / vops);
    return 0;
}

int main(int argc, char** argv)
{
    const int iters = argc > 1 ? atoi(argv[1]) : 200000;
    hipDeviceProp_t p;
    CHECK(hipGetDeviceProperties(&p, 0));
    const int blocks = p.multiProcessorCount * 5;
    int clock_khz = 0;
    CHECK(hipDeviceGetAttribute(&clock_khz, hipDeviceAttributeWallClockRate, 0));
    int per_cu = 0;
    CHECK(hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, k_stream<1>, 256, kLdsBallast));
    float *out, *in; unsigned long long* cyc;
    CHECK(hipMalloc(&out, (size_t)blocks * 256 * 4)); CHECK(hipMalloc(&in, 256 * 4)); CHECK(hipMalloc(&cyc, (size_t)blocks * 8));
    std::vector<float> ones(256, 1.0f);
    CHECK(hipMemcpy(in, ones.data(), 256 * 4, hipMemcpyHostToDevice));
    printf("# %s, %d CUs, grid %d x 256 (five workgroups per CU; the runtime allows %d), %d iterations of a 16-multiply block, wall clock %d kHz\n", p.name, p.multiProcessorCount, blocks, per_cu, iters, clock_khz);
    printf("| mode | stream per block (16 fp32 multiplies) | VALU instructions | ms per launch (median of 5) | min | SIMD ns per block and wave | SIMD ns per instruction |\n|---|---|---|---|---|---|---|\n");
    if (run<0>("16 v_mul_f32", 16, blocks, iters, out, in, cyc, clock_khz)) return 1;
    if (run<1>("8 v_pk_mul_f32", 8, blocks, iters, out, in, cyc, clock_khz)) return 1;
    if (run<2>("8 x (v_mov_b32 + v_pk_mul_f32)", 16, blocks, iters, out, in, cyc, clock_khz)) return 1;
    if (run<3>("8 x (2 v_mov_b32 + v_pk_mul_f32)", 24, blocks, iters, out, in, cyc, clock_khz)) return 1;
    if (run<4>("16 v_mov_b32", 16, blocks, iters, out, in, cyc, clock_khz)) return 1;
    CHECK(hipFree(out)); CHECK(hipFree(in)); CHECK(hipFree(cyc));
    return 0;
}
