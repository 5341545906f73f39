/*
 * atomic_rate.hip -- what a device-scope atomicAdd costs on gfx950 when many wavefronts issue it on the same word, on words of
 * one 128-byte line, or on words spread over 8 / 64 / 256 lines: the shared resource behind the work counters (DevCounters,
 * flush_counters: one flush per wavefront of k_optimize) and the list claims of k_generate (one returning atomicAdd per
 * workgroup on round_work[r]).  profiles/atomic_rate.txt is its output; profiles/round_atomics.md puts it next to the trace.
 *
 *   hipcc --offload-arch=gfx950 -O3 -o /tmp/atomic_rate tools/ubench/atomic_rate.hip && /tmp/atomic_rate
 *
 * One wavefront per workgroup, as k_optimize.  A wavefront runs `work` dependent v_fma_f32 (0: none; 2000: a few microseconds,
 * the life of a short patch wavefront) and then lane 0 issues PER atomics: atomic k of workgroup b goes to byte
 * (b % TARGETS) * target_stride + k * k_stride of the buffer.  Reported per case: the launch with the atomics, the same launch
 * without them, and the difference per atomic -- what the atomics add to the launch, which is 0 if they retire in the shadow of
 * the ALU work and the same-word rate if the launch cannot end before they have drained.
 */
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>

template <typename T, bool RET, int PER>
__global__ __launch_bounds__(64) void k_atomic(T* __restrict__ buf, unsigned* __restrict__ sink, unsigned work, unsigned targets,
                                               unsigned target_stride, unsigned k_stride, int with_atomics) {
    float f = __uint_as_float(0x3F800000u | (blockIdx.x & 0xFFu));
    for (unsigned q = 0; q < work; ++q) asm volatile("v_fma_f32 %0, %0, %0, %0" : "+v"(f));
    unsigned acc = __float_as_uint(f);
    if (threadIdx.x == 0 && with_atomics) {
        char* base = reinterpret_cast<char*>(buf) + (size_t)(blockIdx.x % targets) * target_stride;
#pragma unroll
        for (int k = 0; k < PER; ++k) {
            T* p = reinterpret_cast<T*>(base + (size_t)k * k_stride);
            if (RET) acc += (unsigned)atomicAdd(p, (T)1);
            else atomicAdd(p, (T)1);
        }
    }
    if (acc == 0x12345678u) sink[0] = acc;       /* (keeps the FMA chain and the returned values alive) */
}

template <typename T, bool RET, int PER>
static double launch_ms(T* buf, unsigned* sink, unsigned grid, unsigned work, unsigned targets, unsigned ts, unsigned ks, int with) {
    hipEvent_t a, b; (void)hipEventCreate(&a); (void)hipEventCreate(&b);
    double best = 1e30;
    for (int rep = 0; rep < 4; ++rep) {                                 /* (the first one warms; the best of the other three) */
        (void)hipEventRecord(a, 0);
        hipLaunchKernelGGL((k_atomic<T, RET, PER>), dim3(grid), dim3(64), 0, 0, buf, sink, work, targets, ts, ks, with);
        (void)hipEventRecord(b, 0); (void)hipEventSynchronize(b);
        float ms = 0; (void)hipEventElapsedTime(&ms, a, b);
        if (rep > 0 && ms < best) best = ms;
    }
    (void)hipEventDestroy(a); (void)hipEventDestroy(b);
    return best;
}

template <typename T, bool RET, int PER>
static void row(const char* what, T* buf, unsigned* sink, unsigned grid, unsigned work, unsigned targets, unsigned ts, unsigned ks) {
    const double t1 = launch_ms<T, RET, PER>(buf, sink, grid, work, targets, ts, ks, 1);
    const double t0 = launch_ms<T, RET, PER>(buf, sink, grid, work, targets, ts, ks, 0);
    printf("%-44s | %6u | %4u | %-3s | %-3s | %d | %9.1f | %9.1f | %8.2f\n", what, grid, work, sizeof(T) == 8 ? "u64" : "u32",
           RET ? "ret" : "no", PER, t1 * 1000.0, t0 * 1000.0, (t1 - t0) * 1e6 / ((double)grid * PER));
}

template <typename T, bool RET>
static void patterns(T* buf, unsigned* sink, unsigned grid, unsigned work) {
    row<T, RET, 1>("one word", buf, sink, grid, work, 1, 0, 0);
    row<T, RET, 1>("4 words of one 128-byte line", buf, sink, grid, work, 4, 32, 0);
    row<T, RET, 1>("8 lines", buf, sink, grid, work, 8, 128, 0);
    row<T, RET, 1>("64 lines", buf, sink, grid, work, 64, 128, 0);
    row<T, RET, 1>("256 lines", buf, sink, grid, work, 256, 128, 0);
}

int main() {
    hipDeviceProp_t p; (void)hipGetDeviceProperties(&p, 0);
    unsigned long long* buf; unsigned* sink;
    const size_t bytes = 256 * 1024;                                     /* 256 stripes of 1 KB at the most */
    if (hipMalloc((void**)&buf, bytes) != hipSuccess || hipMalloc((void**)&sink, 64) != hipSuccess) { printf("alloc failed\n"); return 1; }
    (void)hipMemset(buf, 0, bytes); (void)hipMemset(sink, 0, 64);
    printf("%d CUs; one wavefront per workgroup, lane 0 issues the atomics after `work` dependent v_fma_f32\n", p.multiProcessorCount);
    printf("%-44s | waves  | work | T   | ret | n | with us   | without   | ns added per atomic\n", "targets");
    const unsigned grids[2] = {3072u, 32768u}, works[2] = {0u, 2000u};
    for (int g = 0; g < 2; ++g)
        for (int w = 0; w < 2; ++w) {
            patterns<unsigned, true>((unsigned*)buf, sink, grids[g], works[w]);
            patterns<unsigned, false>((unsigned*)buf, sink, grids[g], works[w]);
            patterns<unsigned long long, true>(buf, sink, grids[g], works[w]);
            patterns<unsigned long long, false>(buf, sink, grids[g], works[w]);
            /* the flush of a k_optimize wavefront: seven u64 adds on one struct (40 bytes apart: four lines, three words in the
             * first), and what the striped form issues: four adds on one of 16 / 64 / 256 stripes of 512 bytes */
            row<unsigned long long, false, 7>("flush: 7 adds, one struct", buf, sink, grids[g], works[w], 1, 0, 40);
            row<unsigned long long, false, 4>("flush: 4 adds, one struct", buf, sink, grids[g], works[w], 1, 0, 64);
            row<unsigned long long, false, 4>("flush: 4 adds, 16 stripes", buf, sink, grids[g], works[w], 16, 512, 64);
            row<unsigned long long, false, 4>("flush: 4 adds, 64 stripes", buf, sink, grids[g], works[w], 64, 512, 64);
            row<unsigned long long, false, 4>("flush: 4 adds, 256 stripes", buf, sink, grids[g], works[w], 256, 512, 64);
        }
    /* the list claim of k_generate: 28 800 workgroups (72 tiles x 400 views) against 7 200 / 3 600 (strips of 4 / 8 tiles), each
     * with one RETURNING add on one word and one more on a word of its view (400 words = 13 lines) */
    printf("\nlist claims: one returning u32 add on one word per workgroup\n");
    row<unsigned, true, 1>("28800 claims (one per tile)", (unsigned*)buf, sink, 28800, 200, 1, 0, 0);
    row<unsigned, true, 1>("7200 claims (strips of 4)", (unsigned*)buf, sink, 7200, 800, 1, 0, 0);
    row<unsigned, true, 1>("3600 claims (strips of 8)", (unsigned*)buf, sink, 3600, 1600, 1, 0, 0);
    hipError_t e = hipDeviceSynchronize();
    if (e != hipSuccess) { printf("error: %s\n", hipGetErrorString(e)); return 1; }
    return 0;
}
