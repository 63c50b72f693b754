// Pitch correction (extension; tvc_pitch_snap_f32 and the tvc_tuned_convert* entries): snap rows of f0 to a table of allowed notes, with
// hysteresis on the choice of the note, a one-pole retune of the correction and a strength.  The definition is in tinyvc_hip.h: fp32, every
// operation rounded on its own (__fmul_rn / __fadd_rn / __fsub_rn / __fdiv_rn, a correctly rounded sqrt), no transcendentals - numpy holds it
// bit for bit (tests/helpers_pitch_snap.py).
// One wavefront per row, four rows per 256-thread workgroup.  The workgroup builds the table once in LDS - the notes up to K, the bounds
// b[i], lo[i] and hi[i] - and its waves part ways behind the one barrier.  A wave walks its row in chunks of 64 frames:
//   1. every lane loads a frame, tests the range and binary-searches near(x) in the bounds;
//   2. the note recursion runs on wave-uniform values, one step per EVENT rather than per frame: while q stands (lo[q] and hi[q] in
//      registers, broadcast from the lane whose near(x) became q) one ballot finds the first frame that leaves the note or the range,
//      every frame in front of it keeps q, and that frame's own near(x) (a lane broadcast) is the next q;
//   3. r = notes[n] / x in all lanes;
//   4. the three-operation c recursion runs serially over the chunk's frames: every lane follows it up to its own frame and keeps c there,
//      so lane j holds c_j and the chunk's last lane the state of the next chunk;
//   5. the outputs are stored in parallel.
// A row of 1 frame and one of 15 000 take this path.  No workspace, no atomics, no host synchronisation: capturable, and out may be f0
// (a lane reads its frame before it writes it).
// MEMORY SAFETY: K is found here, from the table as it stands when the kernel runs, and every index into the table comes from near(x) <
// K or from a prior that passed 0 <= note < K - whatever a caller wrote into notes or into the state.
#include <cmath>
#include <cstdint>

#include "tvc_common.h"

namespace tvc {

constexpr int kSnapWaves = 4;                       // rows per workgroup
constexpr float kSnapRatioMin = 0.6666667f;         // 2/3f = 0x3F2AAAAB
constexpr float kSnapRatioMax = 1.5f;
static_assert(TVC_PITCH_SNAP_NOTES == 128, "the table build below takes two wavefronts");

// the rows of one launch by value: row i = columns [start, start + len) of f0, idx = its slot in strength and the state
struct SnapRows {
    int start[SNAP_ROWS], len[SNAP_ROWS], idx[SNAP_ROWS];
};
struct SnapState {
    int32_t* note;        // nullable, with ratio
    float* ratio;
    int frame;            // the state is stored behind frame `frame - 1`
};

// uniform_len >= 0: row i = columns [rows.start[0] + i * uniform_len, + uniform_len), idx = rows.idx[0] + i - any number of rows in one launch
static __global__ __launch_bounds__(256) void pitch_snap_kernel(SnapRows rows, int nrows, int uniform_len, const float* f0, const float* __restrict__ notes,
                                                                const float* __restrict__ strength, float h, float g, float f_min, float f_max, SnapState st,
                                                                float* out, int32_t* note_out) {
    __shared__ float nt[TVC_PITCH_SNAP_NOTES], bd[TVC_PITCH_SNAP_NOTES], lo[TVC_PITCH_SNAP_NOTES], hi[TVC_PITCH_SNAP_NOTES];
    __shared__ int bad[2];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    // ---- the table: K, then b, lo and hi
    if (tid < TVC_PITCH_SNAP_NOTES) {
        const float v = notes[tid];
        nt[tid] = v;
        const float before = tid > 0 ? notes[tid - 1] : 0.f;
        const bool ok = fabsf(v) < INFINITY && v > before;      // finite, notes[0] > 0, strictly ascending (NaN fails both)
        const unsigned long long m = __ballot(!ok);
        if (lane == 0) bad[wave] = m ? __ffsll((long long)m) - 1 : 64;
    }
    __syncthreads();
    const int K = bad[0] < 64 ? bad[0] : 64 + bad[1];
    if (tid < TVC_PITCH_SNAP_NOTES) bd[tid] = tid < K - 1 ? sqrtf(__fmul_rn(nt[tid], nt[tid + 1])) : INFINITY;
    __syncthreads();
    if (tid < TVC_PITCH_SNAP_NOTES) {
        lo[tid] = tid > 0 && tid < K ? __fdiv_rn(bd[tid - 1], h) : 0.f;
        hi[tid] = tid < K - 1 ? __fmul_rn(bd[tid], h) : INFINITY;
    }
    __syncthreads();
    // ---- one wave, one row: no barrier from here on
    const int row = blockIdx.x * kSnapWaves + wave;
    if (row >= nrows) return;
    const int len = uniform_len >= 0 ? uniform_len : rows.len[row];
    if (len <= 0) return;
    const long start = uniform_len >= 0 ? (long)rows.start[0] + (long)row * uniform_len : (long)rows.start[row];
    const long idx = uniform_len >= 0 ? (long)rows.idx[0] + row : (long)rows.idx[row];
    float s = strength ? strength[idx] : 1.f;
    s = s != s ? 0.f : fminf(fmaxf(s, 0.f), 1.f);
    int q = -1;
    float c = 1.f;
    if (st.note) {      // a prior counts only if it names a note of this table and a ratio inside the clamp
        const int pn = st.note[idx];
        const float pc = st.ratio[idx];
        if (pn >= 0 && pn < K && kSnapRatioMin <= pc && pc <= kSnapRatioMax) {
            q = pn;
            c = pc;
        }
    }
    q = __builtin_amdgcn_readfirstlane(q);
    float qlo = q >= 0 ? lo[q] : 0.f, qhi = q >= 0 ? hi[q] : 0.f;
    const int nb = K > 0 ? K - 1 : 0;      // bounds in the table
    float ahead = lane < len ? f0[start + lane] : 0.f;      // the next chunk's frames are loaded while this one is walked
    for (int t0 = 0; t0 < len; t0 += 64) {
        const int m = min(64, len - t0);
        const bool mine = lane < m;
        // 1. load, range, near(x)
        const float x = ahead;
        if (t0 + 64 < len) ahead = t0 + 64 + lane < len ? f0[start + t0 + 64 + lane] : 0.f;
        const bool inr = mine && K > 0 && f_min <= x && x <= f_max;
        int nr = 0;
#pragma unroll
        for (int step = 64; step; step >>= 1)
            if (nr + step <= nb && bd[nr + step - 1] <= x) nr += step;
        const float mylo = lo[nr], myhi = hi[nr];      // (nr <= 127) what q = nr would hold: the serial part below reads no LDS
        // 2. the note recursion, event by event
        int n = -1;
        bool fresh = false;
        const unsigned long long in_mask = __ballot(inr);
        unsigned long long todo = m == 64 ? ~0ull : (1ull << m) - 1;
        while (todo) {
            const unsigned long long me = 1ull << lane;
            if (q >= 0) {
                const unsigned long long stay = __ballot(inr && qlo < x && x < qhi);
                const unsigned long long brk = todo & ~stay;
                const int j = brk ? __ffsll((long long)brk) - 1 : 64;
                const unsigned long long run = j < 64 ? todo & ((1ull << j) - 1) : todo;
                if (run & me) n = q;
                todo &= ~run;
                if (j == 64) break;
                q = (in_mask >> j) & 1 ? __builtin_amdgcn_readlane(nr, j) : -1;      // the frame changes the note, or leaves the range
                if (lane == j) n = q;
                todo &= ~(1ull << j);
                qlo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mylo), j));
                qhi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myhi), j));
            } else {
                const unsigned long long first = todo & in_mask;
                const int j = first ? __ffsll((long long)first) - 1 : 64;
                todo &= j < 64 ? ~((1ull << j) - 1) : 0ull;      // the frames in front of it stay out: n = -1
                if (j == 64) break;
                q = __builtin_amdgcn_readlane(nr, j);
                if (lane == j) {
                    n = q;
                    fresh = true;      // a note starts in tune
                }
                todo &= ~(1ull << j);
                qlo = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, mylo), j));
                qhi = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, myhi), j));
            }
        }
        // 3. r in parallel
        const float r = n >= 0 ? __fdiv_rn(nt[n], x) : 1.f;
        // 4. the c recursion: lane l follows frames 0 .. l and keeps c_l
        const unsigned long long fresh_mask = __ballot(fresh);
        for (int j = 0; j < m; ++j) {
            if (!((in_mask >> j) & 1)) continue;
            const float rj = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, r), j));
            float cn = (fresh_mask >> j) & 1 ? rj : __fadd_rn(c, __fmul_rn(g, __fsub_rn(rj, c)));
            cn = fminf(fmaxf(cn, kSnapRatioMin), kSnapRatioMax);
            c = j <= lane ? cn : c;
        }
        // 5. the outputs
        if (mine) {
            out[start + t0 + lane] = n >= 0 ? __fmul_rn(x, __fadd_rn(1.f, __fmul_rn(s, __fsub_rn(c, 1.f)))) : x;
            if (note_out) note_out[start + t0 + lane] = n;
            if (st.note && t0 + lane == st.frame - 1) {
                st.note[idx] = n;
                st.ratio[idx] = n >= 0 ? c : 1.f;
            }
        }
        c = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 63));      // lanes behind the row's end followed every frame too
    }
}

// 0, or TVC_ERR_ARG with the reason in `why`
int pitch_snap_check(const tvc_pitch_snap& p, char* why, size_t why_bytes) {
    auto refuse = [&](const char* fmt, double v, double w) {
        if (why && why_bytes) snprintf(why, why_bytes, fmt, v, w);
        return (int)TVC_ERR_ARG;
    };
    if (!(p.hysteresis >= 1.f && p.hysteresis <= kSnapMaxHysteresis))
        return refuse("hysteresis = %g is outside 1 .. 2^(1/12) = %g (a frequency ratio)", (double)p.hysteresis, (double)kSnapMaxHysteresis);
    if (!(p.retune > 0.f && p.retune <= 1.f)) return refuse("retune = %g is outside (0, 1] (the per-frame coefficient of the smoother)", (double)p.retune, 0.0);
    if (!(p.f_min >= 32.f) || !std::isfinite(p.f_min) || !std::isfinite(p.f_max) || !(p.f_min <= p.f_max))
        return refuse("f_min = %g, f_max = %g: need 32 <= f_min <= f_max, both finite", (double)p.f_min, (double)p.f_max);
    if (why && why_bytes) why[0] = 0;
    return 0;
}

int run_pitch_snap(tvc_ctx* ctx, hipStream_t s, const float* f0, const std::vector<SnapRow>& rows, const tvc_pitch_snap& p, const float* notes,
                   const float* strength, int carry_frame, int32_t* note, float* ratio, float* out, int32_t* note_out) {
    const SnapState st{note && ratio ? note : nullptr, note && ratio ? ratio : nullptr, carry_frame};
    const size_t n = rows.size();
    bool uniform = n > 0 && (int64_t)rows[0].start + (int64_t)n * rows[0].len <= 0x7fffffff;
    for (size_t i = 1; uniform && i < n; ++i)
        uniform = rows[i].len == rows[0].len && rows[i].start == rows[0].start + (int64_t)i * rows[0].len && rows[i].idx == rows[0].idx + (int64_t)i;
    SnapRows r = {};
    if (uniform) {      // equal rows back to back (a batch, a set of streams): one launch however many
        r.start[0] = rows[0].start;
        r.idx[0] = rows[0].idx;
        hipLaunchKernelGGL(pitch_snap_kernel, dim3((unsigned)((n + kSnapWaves - 1) / kSnapWaves)), dim3(256), 0, s, r, (int)n, rows[0].len, f0, notes, strength,
                           p.hysteresis, p.retune, p.f_min, p.f_max, st, out, note_out);
        return launch_check(ctx, "pitch_snap");
    }
    for (size_t o = 0; o < n; o += SNAP_ROWS) {
        const int k = (int)(n - o < SNAP_ROWS ? n - o : SNAP_ROWS);
        for (int i = 0; i < k; ++i) {
            r.start[i] = rows[o + i].start;
            r.len[i] = rows[o + i].len;
            r.idx[i] = rows[o + i].idx;
        }
        hipLaunchKernelGGL(pitch_snap_kernel, dim3((unsigned)((k + kSnapWaves - 1) / kSnapWaves)), dim3(256), 0, s, r, k, -1, f0, notes, strength, p.hysteresis,
                           p.retune, p.f_min, p.f_max, st, out, note_out);
    }
    return launch_check(ctx, "pitch_snap");
}

}  // namespace tvc
