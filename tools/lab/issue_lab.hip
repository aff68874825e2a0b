// issue_lab: the issue time of a few VALU instructions against v_and_b32 — what k_pack_b's pair index (v_dot4_u32_u8) and its
// emission (v_lshlrev_b64) cost per instruction. Runs of independent instructions (eight chains per lane), every SIMD busy.
// hipcc --offload-arch=gfx950 -O3 -o issue_lab issue_lab.hip ; ./issue_lab
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdint.h>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); return 1; } } while (0)
#define THREADS 512
#define BLOCKS 1024
#define TRIPS 2048
#define PER_TRIP 32  // instructions of a trip: four rounds over the eight chains

enum { OP_AND, OP_SHL32, OP_SHL64, OP_DOT4, OP_MAD24, OP_BFE, OP_COUNT };
static const char *NAMES[OP_COUNT] = {"v_and_b32", "v_lshlrev_b32", "v_lshlrev_b64", "v_dot4_u32_u8", "v_mad_u32_u24", "v_bfe_u32"};

#define ROUND32(INS) asm volatile(INS(0) INS(1) INS(2) INS(3) INS(4) INS(5) INS(6) INS(7) \
                                  : "+v"(a[0]), "+v"(a[1]), "+v"(a[2]), "+v"(a[3]), "+v"(a[4]), "+v"(a[5]), "+v"(a[6]), "+v"(a[7]) : "v"(b), "v"(c))
#define ROUND64(INS) asm volatile(INS(0) INS(1) INS(2) INS(3) INS(4) INS(5) INS(6) INS(7) \
                                  : "+v"(q[0]), "+v"(q[1]), "+v"(q[2]), "+v"(q[3]), "+v"(q[4]), "+v"(q[5]), "+v"(q[6]), "+v"(q[7]) : "v"(b), "v"(c))
#define I_AND(k) "v_and_b32 %" #k ", %8, %" #k "\n"
#define I_SHL32(k) "v_lshlrev_b32 %" #k ", %9, %" #k "\n"
#define I_SHL64(k) "v_lshlrev_b64 %" #k ", %9, %" #k "\n"
#define I_DOT4(k) "v_dot4_u32_u8 %" #k ", %8, %9, %" #k "\n"
#define I_MAD24(k) "v_mad_u32_u24 %" #k ", %8, %9, %" #k "\n"
#define I_BFE(k) "v_bfe_u32 %" #k ", %" #k ", %9, %8\n"

template <int OP>
__global__ __launch_bounds__(THREADS) void k_issue(uint32_t *out, uint32_t b, uint32_t c) {
    uint32_t a[8];
    uint64_t q[8];
    for (int k = 0; k < 8; k++) {
        a[k] = threadIdx.x * 2654435761u + k;
        q[k] = ((uint64_t)a[k] << 32) | (blockIdx.x + k);
    }
    for (int t = 0; t < TRIPS; t++) {
#pragma unroll
        for (int r = 0; r < PER_TRIP / 8; r++) {
            if (OP == OP_AND) ROUND32(I_AND);
            if (OP == OP_SHL32) ROUND32(I_SHL32);
            if (OP == OP_SHL64) ROUND64(I_SHL64);
            if (OP == OP_DOT4) ROUND32(I_DOT4);
            if (OP == OP_MAD24) ROUND32(I_MAD24);
            if (OP == OP_BFE) ROUND32(I_BFE);
        }
    }
    uint32_t s = 0;
    for (int k = 0; k < 8; k++) s ^= a[k] ^ (uint32_t)q[k] ^ (uint32_t)(q[k] >> 32);
    out[(size_t)blockIdx.x * THREADS + threadIdx.x] = s;
}

typedef void (*kern)(uint32_t *, uint32_t, uint32_t);

int main() {
    uint32_t *out;
    CK(hipMalloc(&out, (size_t)BLOCKS * THREADS * sizeof(uint32_t)));
    kern ks[OP_COUNT] = {k_issue<OP_AND>, k_issue<OP_SHL32>, k_issue<OP_SHL64>, k_issue<OP_DOT4>, k_issue<OP_MAD24>, k_issue<OP_BFE>};
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    float best[OP_COUNT];
    for (int op = 0; op < OP_COUNT; op++) {
        best[op] = 1e30f;
        for (int rep = 0; rep < 6; rep++) {  // (the first is the warm-up)
            CK(hipEventRecord(e0));
            hipLaunchKernelGGL(ks[op], dim3(BLOCKS), dim3(THREADS), 0, 0, out, 0xFFFFFF0Fu, 1u);
            CK(hipEventRecord(e1));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            if (rep && ms < best[op]) best[op] = ms;
        }
        CK(hipGetLastError());
    }
    const double wave_instr = (double)BLOCKS * (THREADS / 64) * TRIPS * PER_TRIP;
    for (int op = 0; op < OP_COUNT; op++)
        printf("%-16s %8.3f ms  %6.2f G wave-instr/s  x%.2f of v_and_b32\n", NAMES[op], best[op], wave_instr / best[op] * 1e-6, best[op] / best[OP_AND]);
    CK(hipFree(out));
    return 0;
}
