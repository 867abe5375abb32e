// What does the kernel boundary in front of the propagation kernel pay for? ("its end -> next propagation kernel starts")
// A predecessor shaped like k_syrk_lift (214 workgroups of 512 threads) and a successor shaped like k_propagate_main (28 workgroups) run back to back on one
// stream; both stamp the device wall clock (100 MHz) the way EQF_OPT_TRACE does: the predecessor keeps the latest finishing time of its workgroups (atomicMax by
// thread 0 of each, behind its stores, not behind their acknowledgement), block 0 / thread 0 of the successor stamps its first instruction. Reported: median of
// (successor's stamp - predecessor's stamp) over PAIRS pairs, one factor toggled at a time from a bare boundary, then each factor removed from the full set:
//   pin    the predecessor's first 4 workgroups write an 8 KB result packet to pinned host memory, fence it at system scope and ring a doorbell word
//          (ring_doorbell of eqf_kernels.hpp): "early" = 5 us before the launch's other workgroups finish (where the lift's doorbell rings), "end" = at the very end
//   karg   bytes of the successor's kernel-argument segment (every 64-byte line of it read by every wave), freshly written by the host for each launch
//   shape  successor small (64 threads, no LDS) or heavy (768 threads, >= 148 VGPRs, 40 KB of LDS)
//   dirty  bytes the predecessor leaves dirty in the L2s (plain 16-byte stores just in front of its end stamp, spread over all workgroups = all XCDs)
//   late   one wave of the predecessor's last workgroup ends 3 us after everybody else
//   query  the host calls hipStreamQuery once between the two launches, as a doorbell wait that also watches the stream does (door_wait of eqf_hip.hip): the
//          runtime then queues a marker with a completion signal behind the predecessor, a barrier packet of its own in front of the successor
//   delay  the host launches the successor this many us after it has SEEN the predecessor start (a pinned word the predecessor sets first): how much
//          lead the launch needs before the predecessor's end (at 15 us; the launch call itself takes the printed time)
// The predecessor spins on the wall clock for 15 us so that the host has queued the successor before it ends; the rows "predecessor X us" vary that lead
// (X minus about the host's time in the successor's launch call, which is printed): a successor queued too late pays the launch path, not the boundary.
// hipcc --offload-arch=gfx950 -O2 kernel_boundary.hip -o kernel_boundary && ./kernel_boundary
#include <hip/hip_runtime.h>
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>
#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("HIP error %s at %d\n", hipGetErrorString(e), __LINE__); return 1; } } while (0)
typedef unsigned long long u64;
constexpr int PAIRS = 3000, WARM = 200;
constexpr int PRED_BLOCKS = 214, PRED_T = 512, PIN_BLOCKS = 4, SUCC_BLOCKS = 28;
constexpr size_t DIRTY_CAP = 4u << 20;
struct PredArgs {
    u64* end;          // latest finishing stamp of the launch
    double* dirty;     // DIRTY_CAP bytes of device memory
    unsigned dirty_bytes;
    int pin;           // 0 none, 1 early, 2 at the end
    double* packet;    // pinned: PIN_BLOCKS * 64 * 4 doubles
    int *door_count, *door_host;
    int seq;
    int* started; // pinned: set to seq by the first thread of the launch (the "delay" rows only)
    unsigned spin_ticks, pin_lead_ticks, late_ticks;
};
__device__ __forceinline__ void spin_until(u64 t0, unsigned ticks) {
    while (wall_clock64() - t0 < ticks)
        __builtin_amdgcn_s_sleep(2);
}
__global__ void __launch_bounds__(PRED_T) k_pred(const PredArgs a) {
    const u64 t0 = wall_clock64();
    const int b = blockIdx.x, tid = threadIdx.x;
    if (a.started && b == 0 && tid == 0)
        *reinterpret_cast<volatile int*>(a.started) = a.seq;
    if (a.pin && b < PIN_BLOCKS) { // the lift's workgroups: first wave only, results to the pinned packet, fence, count, doorbell
        if (tid >= 64)
            return;
        spin_until(t0, a.pin == 1 && a.spin_ticks > a.pin_lead_ticks ? a.spin_ticks - a.pin_lead_ticks : a.spin_ticks);
        for (int pl = 0; pl < 4; ++pl)
            a.packet[pl * (PIN_BLOCKS * 64) + b * 64 + tid] = (double)(a.seq + pl);
        __threadfence_system();
        if (tid == 0) {
            if (atomicAdd(a.door_count, 1) == PIN_BLOCKS - 1) {
                atomicExch(a.door_count, 0);
                __threadfence_system();
                *reinterpret_cast<volatile int*>(a.door_host) = a.seq;
            }
            atomicMax(a.end, (u64)wall_clock64());
        }
        return;
    }
    spin_until(t0, a.spin_ticks);
    const unsigned per = (a.dirty_bytes / gridDim.x) / 16; // 16-byte stores of this workgroup: (b + 1) * per * 16 <= dirty_bytes <= DIRTY_CAP
    double2* mine = reinterpret_cast<double2*>(a.dirty) + (size_t)b * per;
    for (unsigned e = tid; e < per; e += PRED_T)
        mine[e] = double2{(double)a.seq, (double)e};
    if (a.late_ticks && b == (int)gridDim.x - 1 && tid < 64)
        spin_until(t0, a.spin_ticks + a.late_ticks);
    if (tid == 0)
        atomicMax(a.end, (u64)wall_clock64());
}
template <int KB> struct SuccArgs {
    unsigned pad[(KB - 24) / 4];
    u64* start;  // block 0's first instruction
    u64* first;  // earliest first instruction of any workgroup
    unsigned* out;
};
template <int KB> __device__ __forceinline__ unsigned read_args(const SuccArgs<KB>& a) {
    unsigned s = 0;
#pragma unroll
    for (int k = 0; k < (KB - 24) / 4; k += 16) // one word of every 64-byte line of the segment
        s += a.pad[k];
    return s;
}
template <int KB> __global__ void __launch_bounds__(64) k_succ_small(const SuccArgs<KB> a) {
    const u64 t = wall_clock64();
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0)
            *a.start = t;
        atomicMin(a.first, t);
    }
    const unsigned s = read_args(a);
    if (threadIdx.x == 0)
        a.out[blockIdx.x] = s;
}
template <int KB> __global__ void __launch_bounds__(768) k_succ_heavy(const SuccArgs<KB> a) {
    const u64 t = wall_clock64();
    __shared__ double sm[5120]; // 40 KB
    if (threadIdx.x == 0) {
        if (blockIdx.x == 0)
            *a.start = t;
        atomicMin(a.first, t);
    }
    asm volatile("v_mov_b32 v147, 0" ::: "v147"); // the register allocation of k_propagate_main (148): what the dispatcher has to find room for
    const unsigned s = read_args(a);
    for (int e = threadIdx.x; e < 5120; e += 768)
        sm[e] = (double)(s + e);
    __syncthreads();
    if (threadIdx.x == 0)
        a.out[blockIdx.x] = s + (unsigned)sm[(s + 17) % 5120];
}
struct Cfg {
    const char* name;
    int pin, karg, heavy;
    unsigned dirty;
    int late, spin_us;
    int query, delay_us; // delay_us < 0: the successor is launched right behind the predecessor
};
template <int KB> static void launch_succ(bool heavy, hipStream_t st, u64* start, u64* first, unsigned* out, unsigned k) {
    SuccArgs<KB> a;
    for (unsigned i = 0; i < sizeof(a.pad) / 4; ++i)
        a.pad[i] = k + i; // fresh bytes for every launch
    a.start = start, a.first = first, a.out = out;
    if (heavy)
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_succ_heavy<KB>), dim3(SUCC_BLOCKS), dim3(768), 0, st, a);
    else
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_succ_small<KB>), dim3(SUCC_BLOCKS), dim3(64), 0, st, a);
}
int main() {
    u64 *d_end, *d_start, *d_first;
    double *d_dirty, *h_packet;
    int *d_count, *h_door, *h_started;
    unsigned* d_out;
    const int total = PAIRS + WARM;
    CK(hipMalloc(&d_end, sizeof(u64) * total));
    CK(hipMalloc(&d_start, sizeof(u64) * total));
    CK(hipMalloc(&d_first, sizeof(u64) * total));
    CK(hipMalloc(&d_dirty, DIRTY_CAP));
    CK(hipMalloc(&d_count, 64));
    CK(hipMalloc(&d_out, sizeof(unsigned) * SUCC_BLOCKS));
    CK(hipHostMalloc(&h_packet, sizeof(double) * PIN_BLOCKS * 64 * 4));
    CK(hipHostMalloc(&h_door, 64));
    CK(hipHostMalloc(&h_started, 64));
    *h_started = 0;
    CK(hipMemset(d_count, 0, 64));
    *h_door = 0;
    hipStream_t st;
    CK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
    const unsigned MB = 1u << 20;
    const Cfg cfgs[] = {
        {"bare boundary", 0, 64, 0, 0, 0, 15, 0, -1},
        {"bare, predecessor 40 us (control)", 0, 64, 0, 0, 0, 40, 0, -1},
        {"+ pin early", 1, 64, 0, 0, 0, 15, 0, -1},
        {"+ pin at the end", 2, 64, 0, 0, 0, 15, 0, -1},
        {"+ karg 1024", 0, 1024, 0, 0, 0, 15, 0, -1},
        {"+ karg 4088", 0, 4088, 0, 0, 0, 15, 0, -1},
        {"+ heavy successor", 0, 64, 1, 0, 0, 15, 0, -1},
        {"+ dirty 0.25 MB", 0, 64, 0, MB / 4, 0, 15, 0, -1},
        {"+ dirty 3 MB", 0, 64, 0, 3 * MB, 0, 15, 0, -1},
        {"+ late wave", 0, 64, 0, 0, 1, 15, 0, -1},
        {"ALL (pin early, 4088, heavy, 3 MB, late)", 1, 4088, 1, 3 * MB, 1, 15, 0, -1},
        {"ALL, predecessor 40 us (control)", 1, 4088, 1, 3 * MB, 1, 40, 0, -1},
        {"ALL, N = 50 form (0.25 MB)", 1, 4088, 1, MB / 4, 1, 15, 0, -1},
        {"ALL, predecessor 10 us", 1, 4088, 1, 3 * MB, 1, 10, 0, -1},
        {"ALL, predecessor 8 us", 1, 4088, 1, 3 * MB, 1, 8, 0, -1},
        {"ALL, predecessor 6 us", 1, 4088, 1, 3 * MB, 1, 6, 0, -1},
        {"ALL, predecessor 4 us", 1, 4088, 1, 3 * MB, 1, 4, 0, -1},
        {"ALL, predecessor 2 us", 1, 4088, 1, 3 * MB, 1, 2, 0, -1},
        {"bare, predecessor 8 us", 0, 64, 0, 0, 0, 8, 0, -1},
        {"bare, predecessor 6 us", 0, 64, 0, 0, 0, 6, 0, -1},
        {"bare, predecessor 4 us", 0, 64, 0, 0, 0, 4, 0, -1},
        {"bare, predecessor 2 us", 0, 64, 0, 0, 0, 2, 0, -1},
        {"ALL - pin", 0, 4088, 1, 3 * MB, 1, 15, 0, -1},
        {"ALL - karg (64)", 1, 64, 1, 3 * MB, 1, 15, 0, -1},
        {"ALL - karg (1024)", 1, 1024, 1, 3 * MB, 1, 15, 0, -1},
        {"ALL - heavy", 1, 4088, 0, 3 * MB, 1, 15, 0, -1},
        {"ALL - dirty", 1, 4088, 1, 0, 1, 15, 0, -1},
        {"ALL - late", 1, 4088, 1, 3 * MB, 0, 15, 0, -1},
        {"ALL, pin at the end", 2, 4088, 1, 3 * MB, 1, 15, 0, -1},
        {"bare boundary (again)", 0, 64, 0, 0, 0, 15, 0, -1},
        {"bare + stream query", 0, 64, 0, 0, 0, 15, 1, -1},
        {"ALL + stream query", 1, 4088, 1, 3 * MB, 1, 15, 1, -1},
        {"ALL, N = 50 form + stream query", 1, 4088, 1, MB / 4, 1, 15, 1, -1},
        {"ALL + stream query, predecessor 40 us", 1, 4088, 1, 3 * MB, 1, 40, 1, -1},
        {"ALL, launch delayed 0 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 0},
        {"ALL, launch delayed 4 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 4},
        {"ALL, launch delayed 8 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 8},
        {"ALL, launch delayed 10 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 10},
        {"ALL, launch delayed 12 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 12},
        {"ALL, launch delayed 14 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 14},
        {"ALL, launch delayed 16 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 16},
        {"ALL, launch delayed 20 us", 1, 4088, 1, 3 * MB, 1, 15, 0, 20},
        {"ALL + stream query, launch delayed 4 us", 1, 4088, 1, 3 * MB, 1, 15, 1, 4},
        {"ALL + stream query, launch delayed 12 us", 1, 4088, 1, 3 * MB, 1, 15, 1, 12},
        {"bare boundary (last)", 0, 64, 0, 0, 0, 15, 0, -1},
    };
    printf("%-48s %8s %8s %8s   %s\n", "predecessor's end -> successor, us", "median", "p10", "p90", "first workgroup anywhere (median); host: us in the two launch calls (median)");
    std::vector<u64> ve(total), vs(total), vf(total);
    std::vector<double> gap, gapf, hp, hs;
    using clk = std::chrono::steady_clock;
    int seq = 0;
    for (const Cfg& c : cfgs) {
        CK(hipMemset(d_end, 0, sizeof(u64) * total));
        CK(hipMemset(d_first, 0xff, sizeof(u64) * total));
        CK(hipMemset(d_start, 0, sizeof(u64) * total));
        for (int k = 0; k < total; ++k) {
            PredArgs p{};
            p.end = d_end + k, p.dirty = d_dirty, p.dirty_bytes = c.dirty, p.pin = c.pin, p.packet = h_packet, p.door_count = d_count, p.door_host = h_door;
            p.seq = ++seq, p.spin_ticks = 100u * c.spin_us, p.pin_lead_ticks = 500, p.late_ticks = c.late ? 300 : 0;
            p.started = c.delay_us >= 0 ? h_started : nullptr;
            const auto h0 = clk::now();
            hipLaunchKernelGGL(k_pred, dim3(PRED_BLOCKS), dim3(PRED_T), 0, st, p);
            if (c.delay_us >= 0) { // (bounded by a second; the stream itself is not looked at: that is the "query" factor)
                while (*(volatile int*)h_started != seq && std::chrono::duration<double>(clk::now() - h0).count() < 1.0) {
                }
                const auto seen = clk::now();
                while (std::chrono::duration<double, std::micro>(clk::now() - seen).count() < c.delay_us) {
                }
            }
            if (c.query)
                (void)hipStreamQuery(st);
            const auto h1 = clk::now();
            if (c.karg == 64)
                launch_succ<64>(c.heavy, st, d_start + k, d_first + k, d_out, k);
            else if (c.karg == 1024)
                launch_succ<1024>(c.heavy, st, d_start + k, d_first + k, d_out, k);
            else
                launch_succ<4088>(c.heavy, st, d_start + k, d_first + k, d_out, k);
            const auto h2 = clk::now();
            if (k == 0)
                hp.clear(), hs.clear();
            hp.push_back(std::chrono::duration<double, std::micro>(h1 - h0).count());
            hs.push_back(std::chrono::duration<double, std::micro>(h2 - h1).count());
            CK(hipStreamSynchronize(st));
            if (c.pin && *(volatile int*)h_door != seq) {
                printf("doorbell of pair %d not seen\n", k);
                return 1;
            }
        }
        CK(hipGetLastError());
        CK(hipMemcpy(ve.data(), d_end, sizeof(u64) * total, hipMemcpyDeviceToHost));
        CK(hipMemcpy(vs.data(), d_start, sizeof(u64) * total, hipMemcpyDeviceToHost));
        CK(hipMemcpy(vf.data(), d_first, sizeof(u64) * total, hipMemcpyDeviceToHost));
        gap.clear(), gapf.clear();
        for (int k = WARM; k < total; ++k) {
            gap.push_back(((double)vs[k] - (double)ve[k]) * 0.01);
            gapf.push_back(((double)vf[k] - (double)ve[k]) * 0.01);
        }
        std::sort(gap.begin(), gap.end());
        std::sort(gapf.begin(), gapf.end());
        std::sort(hp.begin(), hp.end());
        std::sort(hs.begin(), hs.end());
        const size_t n = gap.size();
        printf("%-48s %8.2f %8.2f %8.2f   %8.2f   %6.2f %6.2f\n", c.name, gap[n / 2], gap[n / 10], gap[n - 1 - n / 10], gapf[n / 2], hp[hp.size() / 2], hs[hs.size() / 2]);
        fflush(stdout);
    }
    return 0;
}
