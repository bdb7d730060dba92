// Assist text (the contract above sbv2_assist, include/sbv2_hip.h): the mean of an assist sequence's DeBERTa features and its blend into the
// word2ph gather.  Two kernels, no atomics; the f64 sum and the f32 blend in the header's order (this file is built with -ffp-contract=off and
// says so again below: no product and sum here may become a fused multiply-add).
#include "ops.h"

#pragma clang fp contract(off)

namespace sbv2 {

// One wavefront per (assist sequence a, channel c): lane l adds the columns l, l + 64, ... of the sequence in ascending order in f64, then the
// lanes fold pairwise (h = 32 .. 1: acc[l] += acc[l + h] for l < h).  The plane is channel-major: a wavefront reads S_a contiguous floats.
__global__ void __launch_bounds__(256) k_assist_mean(Plane F, const int* __restrict__ a_start, const int* __restrict__ a_len, int A, float* __restrict__ mean) {
    const int lane = threadIdx.x & 63;
    const int cpb = (F.C + 3) >> 2;                       // blocks per sequence: four channels (wavefronts) each
    const int a = blockIdx.x / cpb;
    const int c = (blockIdx.x % cpb) * 4 + (threadIdx.x >> 6);
    if (a >= A || c >= F.C) return;                        // (whole wavefronts leave: the shuffles below see all 64 lanes)
    const int s0 = a_start[a], S = a_len[a];
    const float* row = F.p + (size_t)c * F.ld + s0;
    double acc = 0.0;
    for (int i = lane; i < S; i += 64) acc = acc + (double)row[i];
    for (int h = 32; h >= 1; h >>= 1) {
        const double o = __shfl_down(acc, h, 64);
        acc = acc + o;                                     // (lanes >= h add what no lower lane reads again)
    }
    if (lane == 0) mean[(size_t)a * F.C + c] = (float)(acc / (double)S);
}
void assist_mean(Plane F, const int* a_start, const int* a_len, int A, float* mean, hipStream_t s) {
    const int cpb = (F.C + 3) >> 2;
    hipLaunchKernelGGL(k_assist_mean, dim3((unsigned)(A * cpb)), dim3(256), 0, s, F, a_start, a_len, A, mean);
}

// gather_cols with the row's assist blended in: a column's row is seg_of[n], its record rows[seg_of[n]]; mean_row < 0 = the plain gather
__global__ void __launch_bounds__(256) k_gather_cols_assist(Plane in, const int* __restrict__ map, const int* __restrict__ seg_of,
                                                            const AssistRow* __restrict__ rows, const float* __restrict__ mean, Plane out) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int c = blockIdx.y;
    if (n >= out.L) return;
    const int q = map[n];
    float v = 0.f;
    if (q >= 0) {
        v = in.p[(size_t)c * in.ld + q];
        const AssistRow r = rows[seg_of[n]];
        if (r.mean_row >= 0) {
            const float a = v * r.omw;
            const float b = mean[(size_t)r.mean_row * in.C + c] * r.wf;
            v = a + b;
        }
    }
    out.p[(size_t)c * out.ld + n] = v;
}
void gather_cols_assist(Plane in, const int* map, const int* seg_of, const AssistRow* rows, const float* mean, Plane out, hipStream_t s) {
    hipLaunchKernelGGL(k_gather_cols_assist, dim3((out.L + 255) / 256, out.C), dim3(256), 0, s, in, map, seg_of, rows, mean, out);
}

}  // namespace sbv2
