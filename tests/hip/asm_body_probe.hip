// One generated body per launch on raw limbs (tests/test_gpu_asm_corners.py): each lane loads its record of 128 words, runs the body
// through the ladder_asm.hip.h wrapper the library uses, and stores every output limb.  Word k of a record is the body's asm operand %k
// in the numbering of tools/asmgen/sim.py (the generator's operand order), so the same record feeds sim.run on the CPU; SQRU's wrapper
// takes a.re, which sim.py never sees, from words 40-44.  Built by fourq_amd/build.py's compile_unit (device listing, register-range
// check, placement), like the library's units; tests/test_asm_probe.py checks that build on the CPU.
#include "ladder_asm.hip.h"

namespace {
using namespace fq;

constexpr int WORDS = 128;
enum Body { DBL, DBLT, ADD, STEP, TAU, UPSILON, CHI, TAUDUAL, R1TOR2, TABLEADD, MULU, SQRU };

template <int B> __device__ Fe2<B> ld(const u32* r, int base) {
    Fe2<B> x;
#pragma unroll
    for (int i = 0; i < 5; i++) { x.re.l[i] = r[base + i]; x.im.l[i] = r[base + 5 + i]; }
    return x;
}
template <int B> __device__ void st(u32* w, int base, const Fe2<B>& x) {
#pragma unroll
    for (int i = 0; i < 5; i++) { w[base + i] = x.re.l[i]; w[base + 5 + i] = x.im.l[i]; }
}
__device__ EntryRegs ld_entry(const u32* r, int base) {
    EntryRegs t;
    t.N = ld<1>(r, base); t.D = ld<1>(r, base + 10); t.E = ld<1>(r, base + 20); t.F = ld<1>(r, base + 30);
    return t;
}
}  // namespace

// 64 threads per block: a budget of 512 VGPRs per lane, so the kernel can own the registers the bodies clobber (up to v255)
extern "C" __global__ void __launch_bounds__(64) fq_asm_body_probe(int body, const u32* in, u32* out, u32 n) {
    const u32 lane = blockIdx.x * blockDim.x + threadIdx.x;
    if (lane >= n) return;
    const u32* r = in + (size_t)lane * WORDS;
    u32* w = out + (size_t)lane * WORDS;
    switch (body) {
    case DBL: case DBLT: case TAU: case UPSILON: case CHI: case TAUDUAL: {
        Fe2<1> X = ld<1>(r, 0), Y = ld<1>(r, 10), Z = ld<1>(r, 20);
        if (body == DBL) dbl_asm(X, Y, Z);
        else if (body == DBLT) { Fe2<1> T; dblt_asm(X, Y, Z, T); st(w, 30, T); }
        else if (body == TAU) tau_asm(X, Y, Z);
        else if (body == UPSILON) upsilon_asm(X, Y, Z);
        else if (body == CHI) chi_asm(X, Y, Z);
        else { Fe2<2> N3, D3; Fe2<1> F3; taudual_asm(X, Y, Z, N3, D3, F3); st(w, 30, N3); st(w, 40, D3); st(w, 50, F3); }
        st(w, 0, X); st(w, 10, Y); st(w, 20, Z);
        break;
    }
    case ADD: case STEP: {
        R1 q;
        q.X = ld<1>(r, 0); q.Y = ld<1>(r, 10); q.Z = ld<1>(r, 20);
        q.Ta = Fe2<4>{}; q.Tb = Fe2<2>{};
        if (body == ADD) add_asm(q, ld<1>(r, 50), ld_entry(r, 60), r[100]);
        else step_asm(q, ld_entry(r, 50), r[90]);
        st(w, 0, q.X); st(w, 10, q.Y); st(w, 20, q.Z); st(w, 30, q.Ta); st(w, 40, q.Tb);
        break;
    }
    case R1TOR2: {
        R1 p;
        p.X = ld<1>(r, 40); p.Y = ld<1>(r, 50); p.Z = ld<1>(r, 60); p.Ta = ld<4>(r, 70); p.Tb = ld<2>(r, 80);
        const R2 e = r1_to_r2_asm(p);
        st(w, 0, e.N); st(w, 10, e.D); st(w, 20, e.E); st(w, 30, e.F);
        break;
    }
    case TABLEADD: {
        R2 q;
        q.N = ld<1>(r, 0); q.D = ld<1>(r, 10); q.E = ld<1>(r, 20); q.F = ld<1>(r, 30);
        table_add_asm(q, ld<2>(r, 40), ld<2>(r, 50), ld<1>(r, 60), ld<1>(r, 70));
        st(w, 0, q.N); st(w, 10, q.D); st(w, 20, q.E); st(w, 30, q.F);
        break;
    }
    case MULU:                                  // fe2_mul_asm<1, 1>: the wrapper computes -a.im (operands 20-24) itself
        st(w, 0, fe2_mul_asm(ld<1>(r, 10), ld<1>(r, 25)));
        break;
    case SQRU: {                                // fe2_sqr_asm<1>: the wrapper computes d, s, t from a.re (words 40-44) and a.im (25-29)
        Fe2<1> a;
#pragma unroll
        for (int i = 0; i < 5; i++) { a.re.l[i] = r[40 + i]; a.im.l[i] = r[25 + i]; }
        st(w, 0, fe2_sqr_asm(a));
        break;
    }
    default:
        break;
    }
}

// host side: copy n records in, run `body` on them, copy n records out.  0 on success, otherwise the first failing hipError_t.
extern "C" __attribute__((visibility("default"))) int fq_asm_body_probe_run(int body, const uint32_t* host_in, uint32_t* host_out, uint32_t n) {
    if (n == 0) return 0;
    if (body < DBL || body > SQRU || !host_in || !host_out) return (int)hipErrorInvalidValue;
    const size_t bytes = (size_t)n * WORDS * sizeof(uint32_t);
    u32 *din = nullptr, *dout = nullptr;
    hipError_t e = hipMalloc(&din, bytes);
    if (e == hipSuccess) e = hipMalloc(&dout, bytes);
    if (e == hipSuccess) e = hipMemcpy(din, host_in, bytes, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemset(dout, 0, bytes);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(fq_asm_body_probe, dim3((n + 63) / 64), dim3(64), 0, 0, body, din, dout, n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();
    if (e == hipSuccess) e = hipMemcpy(host_out, dout, bytes, hipMemcpyDeviceToHost);
    const hipError_t f1 = din ? hipFree(din) : hipSuccess;
    const hipError_t f2 = dout ? hipFree(dout) : hipSuccess;
    if (e == hipSuccess) e = f1 != hipSuccess ? f1 : f2;
    return (int)e;
}
