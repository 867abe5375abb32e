// EQF_OPT_INNOVATION_STATS: what the host (eqf_hip.hip) and the kernel (eqf_innovation.hip) share. The kernel is a translation unit - and so a code object - of its
// own: the code object of eqf_hip.hip, every existing kernel in it, is byte for byte what it is without the option.
#pragma once
#include <hip/hip_runtime.h>

namespace eqf {

// EQF_OPT_INNOVATION_STATS: dof, NIS = |z|^2 and log det S = 2 sum log L_jj of the update whose factorisation [L ; W ; z^T] is in memory, one launch of one workgroup behind
// the tail. z is the last row of W (both forms of the factorisation leave it there); L_jj comes from the diagonal of the panels' inverse factor tiles (1 / L_jj; the identity
// padding of a ragged last tile is never read: only columns < m are). `tiles` is the look-ahead kernel's published array or the launch chain's per-panel one - the same layout,
// tile p at 1024 p, [r + 32 c]. Columns of discarded measurements (eqf_stats_select_update: decoupled, (0, R_jj, 0)) are left out through the outlier decision's own verdict,
// removed[lmidx[j / 2]]; with the live columns in front these are exactly the columns behind the last live one, so nothing behind the last factorised panel is read.
// Fixed order: lane t owns the columns t, t + 256, ..; one butterfly per wave (the pairing depends on the lane numbers alone); the four waves' sums in wave order.
struct alignas(32) InnovSlot {
    double nis, logdet;
    int dof, seq; // seq is written last, behind a system-scope fence: the host takes the slot when it shows the launch's number
};
struct InnovArgs {
    int m, rows, ldz;
    const double* W;
    const double* tiles;
    const int* lmidx;   // measurement -> landmark (read only with `removed`)
    const int* removed; // the outlier decision's flags by landmark (pinned), or nullptr: every column is live
    int nlm;            // landmarks `removed` covers (an index outside it counts as live)
    const int* spec;    // the tail's cancellation word, or nullptr
    int spec_seq;
    const int* flags;   // [3] == stall_seq: the look-ahead launch in front gave up (the tiles are not this update's; the retry reports)
    int stall_seq;
    InnovSlot* out;
    int seq;
};
constexpr int INNOV_T = 256;
// one launch of one workgroup on `stream` (eqf_innovation.hip)
void launch_innovation_kernel(const InnovArgs& a, hipStream_t stream);

} // namespace eqf
