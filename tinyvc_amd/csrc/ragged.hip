// Host side of ragged batches (ragged.h): the per-call tables (frames per utterance, their prefix, frame -> utterance, per-launch
// column-tile prefixes) are built on the device from lengths that travel as kernel ARGUMENTS - asynchronous on the caller's stream,
// no host staging buffer to keep alive, capturable.  Behind them, how a call is cut into batches and the loops that run them.
#include "ragged.h"
#include "tvc_common.h"

namespace tvc {

namespace {
struct IntChunk {
    int v[960];
};
__global__ void upload_ints_kernel(IntChunk c, int* __restrict__ dst, int n) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) dst[i] = c.v[i];
}
// one workgroup: pre = exclusive prefix of tb * mult_num / bn (bn = 0: of tb itself), pre[B] = total; col2b (optional) = utterance of every frame
__global__ __launch_bounds__(1024) void rag_prefix_kernel(const int* __restrict__ tb, int* pre, int* __restrict__ col2b, int B, int mult, int bn) {
    __shared__ int part[16];
    __shared__ int carry_s;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (tid == 0) carry_s = 0;
    __syncthreads();
    for (int base = 0; base < B; base += 1024) {
        const int b = base + tid;
        int v = 0;
        if (b < B) v = bn > 0 ? (tb[b] * mult + bn - 1) / bn : tb[b];
        int inc = v;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const int u = __shfl_up(inc, o);
            if (lane >= o) inc += u;
        }
        if (lane == 63) part[wave] = inc;
        __syncthreads();
        int woff = 0;
        for (int w = 0; w < wave; ++w) woff += part[w];
        const int carry = carry_s;
        const int excl = carry + woff + inc - v;
        if (b < B) pre[b] = excl;
        __syncthreads();
        if (tid == 1023) carry_s = carry + woff + inc;
        __syncthreads();
    }
    if (tid == 0) pre[B] = carry_s;
    if (col2b) {      // frame -> utterance: every thread looks its frames' utterance up in the finished prefix (a 26-minute utterance must not be one thread's loop)
        __syncthreads();
        __threadfence_block();
        const int total = carry_s;
        for (int f = tid; f < total; f += 1024) {
            int lo = 0, hi = B - 1;           // last b with pre[b] <= f
            while (lo < hi) {
                const int mid = (lo + hi + 1) >> 1;
                if (pre[mid] <= f) lo = mid;
                else hi = mid - 1;
            }
            col2b[f] = lo;
        }
    }
}
}  // namespace

int upload_ints(tvc_ctx* ctx, hipStream_t s, const std::vector<int>& src, int* dst) {
    for (size_t o = 0; o < src.size(); o += 960) {
        IntChunk c;
        const int n = (int)(src.size() - o < 960 ? src.size() - o : 960);
        std::memcpy(c.v, src.data() + o, (size_t)n * sizeof(int));
        hipLaunchKernelGGL(upload_ints_kernel, dim3((n + 255) / 256), dim3(256), 0, s, c, dst + o, n);
    }
    return launch_check(ctx, "rag upload");
}

int rag_setup(tvc_ctx* ctx, hipStream_t s, Ws& ws, RagHost& h, const std::vector<int>& frames, const std::vector<int>& rows, int Tmax) {
    h.B = (int)frames.size();
    h.tb = frames;
    h.row = rows;
    h.Tmax = Tmax;
    h.pre.assign(h.B + 1, 0);
    h.Tlong = 0;
    h.Tshort = h.B ? frames[0] : 0;
    for (int b = 0; b < h.B; ++b) {
        h.pre[b + 1] = h.pre[b] + frames[b];
        if (frames[b] > h.Tlong) h.Tlong = frames[b];
        if (frames[b] < h.Tshort) h.Tshort = frames[b];
    }
    h.Ttot = h.pre[h.B];
    int* p = ws.get<int>(rag_scratch_ints(h.B, h.Ttot));
    int* d_tb = p;
    p += h.B + 1;
    int* d_pre = p;
    p += h.B + 1;
    int* d_row = p;
    p += h.B + 1;
    int* d_col2b = p;
    p += h.Ttot;
    h.d_pool = p;
    h.pool_slots = kRagTabSlots;
    h.tabs.clear();
    h.d_tb = d_tb;
    h.d_pre = d_pre;
    h.d_row = d_row;
    h.d_col2b = d_col2b;
    if (ws.dry) return 0;
    TVC_CHECK(upload_ints(ctx, s, frames, d_tb));
    TVC_CHECK(upload_ints(ctx, s, rows, d_row));
    hipLaunchKernelGGL(rag_prefix_kernel, dim3(1), dim3(1024), 0, s, d_tb, d_pre, d_col2b, h.B, 1, 0);
    return launch_check(ctx, "rag tables");
}

int rag_min_len(const tvc_ctx* ctx, int len) { return ctx->rag ? ctx->rag->Tshort * (len / ctx->rag->Ttot) : len; }

int rag_view(tvc_ctx* ctx, hipStream_t s, int mult, int bn, RagDev* out, int* ntiles) {
    *out = RagDev{};
    RagHost* h = ctx->rag;
    if (!h) return 0;
    out->tb = h->d_tb;
    out->pre = h->d_pre;
    out->col2b = h->d_col2b;
    out->row = h->d_row;
    out->B = h->B;
    out->mult = mult;
    out->Tmax = h->Tmax;
    if (bn <= 0) return 0;
    for (auto& t : h->tabs)
        if (t.mult == mult && t.bn == bn) {
            out->ts = t.d;
            if (ntiles) *ntiles = t.total;
            return 0;
        }
    if ((int)h->tabs.size() >= h->pool_slots) return fail(ctx, TVC_ERR_STATE, "ragged batch: out of column-tile tables");
    int* d = h->d_pool + (size_t)h->tabs.size() * (h->B + 1);
    int total = 0;
    for (int b = 0; b < h->B; ++b) total += (h->tb[b] * mult + bn - 1) / bn;
    hipLaunchKernelGGL(rag_prefix_kernel, dim3(1), dim3(1024), 0, s, h->d_tb, d, (int*)nullptr, h->B, mult, bn);
    TVC_CHECK(launch_check(ctx, "rag tile table"));
    h->tabs.push_back({mult, bn, total, d});
    out->ts = d;
    if (ntiles) *ntiles = total;
    return 0;
}

int rag_tiles(tvc_ctx* ctx, hipStream_t s, int B, long len, int bn, RagDev* out, int* ntiles, const char* what, int mult) {
    if (const RagHost* h = ctx->rag) {
        if (B != 1 || (mult ? len != (long)h->Ttot * mult : len % h->Ttot != 0))
            return fail(ctx, TVC_ERR_STATE, "%s: a ragged batch runs as one long utterance", what);
        if (!mult) mult = (int)(len / h->Ttot);
    }
    return rag_view(ctx, s, mult, bn, out, ntiles);
}

// ---- the batches of a call (ragged.h) ---------------------------------------------------------------------------------------------
namespace {
// the drivers called inside this scope run for the batch h (ctx->rag); whatever way the scope is left, the context forgets it
struct RagScope {
    tvc_ctx* ctx;
    RagScope(tvc_ctx* c, RagHost* h) : ctx(c) { ctx->rag = h; }
    ~RagScope() { ctx->rag = nullptr; }
};
}  // namespace

int ragged_split(tvc_ctx* ctx, int cap, int B, int64_t Lmax, const int64_t* lens, std::vector<RagBatchPlan>* batches, bool classes) {
    std::vector<RagBatchPlan> open(4);          // the batch being filled, per class
    const int max_frames = cap > 0 && cap < kRagMaxFrames ? cap : kRagMaxFrames;
    for (int b = 0; b < B; ++b) {
        if (lens[b] <= 0 || lens[b] % kHop || lens[b] > Lmax || lens[b] < kNfft / 2 + 1)
            return fail(ctx, TVC_ERR_ARG, "ragged batch: lens[%d] = %lld must be a multiple of 480 in (960, Lmax]", b, (long long)lens[b]);
        const int T = (int)(lens[b] / kHop);
        if (T > kRagMaxFrames) return fail(ctx, TVC_ERR_ARG, "ragged batch: lens[%d] = %lld is longer than a batch may be; convert it with tvc_convert_f32", b, (long long)lens[b]);
        const int cls = classes ? (T >= kRagClassBounds[0]) + (T >= kRagClassBounds[1]) + (T >= kRagClassBounds[2]) : 0;      // (the encoder's kernels make no length-dependent choice: one class)
        RagBatchPlan& p = open[cls];
        if (p.Ttot + T > max_frames && !p.rows.empty()) {
            batches->push_back(p);
            p = RagBatchPlan();
        }
        p.rows.push_back(b);
        p.frames.push_back(T);
        p.Ttot += T;
    }
    for (int c = 3; c >= 0; --c)
        if (!open[c].rows.empty()) batches->push_back(open[c]);
    return 0;
}

int convert_ragged_batches(tvc_ctx* ctx, hipStream_t s, Ws& ws, const std::vector<RagBatchPlan>& batches, const ConvertCall& c) {
    for (auto& p : batches) {
        ws.release(0);
        RagHost h;
        TVC_CHECK(rag_setup(ctx, s, ws, h, p.frames, p.rows, (int)(c.L / kHop)));
        ConvertCall one = c;      // the batch as one long utterance; the kernels find the rows of c.wav / c.wave through h.row
        one.B = 1;
        one.L = (int64_t)p.Ttot * kHop;
        one.lens = nullptr;
        RagScope in_batch(ctx, &h);
        TVC_CHECK(convert_impl(ctx, s, ws, one));
    }
    return 0;
}

namespace {
// packed[c][gpre[row of b] + t'] = batch[c][pre[b] + t'] (c = 768: the f0 row): a later batch's columns into the call's packed outputs
__global__ __launch_bounds__(256) void pack_batch_kernel(const float* __restrict__ ssl_b, const float* __restrict__ f0_b, float* __restrict__ ssl,
                                                         float* __restrict__ f0, RagDev rg, const int* __restrict__ gpre, int Ttot, long S) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= Ttot) return;
    const int b = rg.col2b[t];
    const long dst = (long)gpre[rg.row[b]] + (t - rg.pre[b]);
    const int c = blockIdx.y;
    if (c < kSslDim) ssl[(long)c * S + dst] = ssl_b[(long)c * Ttot + t];
    else f0[dst] = f0_b[t];
}
}  // namespace

int encode_ragged_batches(tvc_ctx* ctx, hipStream_t s, Ws& ws, const std::vector<RagBatchPlan>& batches, const std::vector<int>& gpre, const float* wav,
                          int64_t Lmax, float* ssl, float* f0, int64_t S) {
    ws.release(0);
    const bool direct = batches.size() == 1;      // one batch holds every row in the caller's order: its layout IS the packed one (row stride S)
    int* d_gpre = nullptr;
    if (!direct) {
        d_gpre = ws.get<int>(gpre.size());
        if (!ws.dry) TVC_CHECK(upload_ints(ctx, s, gpre, d_gpre));
    }
    const size_t m0 = ws.mark();
    for (auto& p : batches) {
        ws.release(m0);
        RagHost h;
        TVC_CHECK(rag_setup(ctx, s, ws, h, p.frames, p.rows, (int)(Lmax / kHop)));
        float* spec = ws.get<float>((size_t)kBins * p.Ttot);
        float* ssl_b = direct ? ssl : ws.get<float>((size_t)kSslDim * p.Ttot);
        float* f0_b = direct ? f0 : ws.get<float>((size_t)p.Ttot);
        RagScope in_batch(ctx, &h);
        TVC_CHECK(run_stft(ctx, s, ws, wav, spec, 1, (int64_t)p.Ttot * kHop));
        TVC_CHECK(run_encoder(ctx, s, ws, spec, ssl_b, f0_b, nullptr, 1, p.Ttot));
        if (!direct && !ws.dry) {
            RagDev rg;
            TVC_CHECK(rag_view(ctx, s, 1, 0, &rg, nullptr));
            hipLaunchKernelGGL(pack_batch_kernel, dim3((unsigned)((p.Ttot + 255) / 256), kSslDim + 1), dim3(256), 0, s, ssl_b, f0_b, ssl, f0, rg, d_gpre, p.Ttot, (long)S);
            TVC_CHECK(launch_check(ctx, "encode_ragged pack"));
        }
    }
    return 0;
}

int encode_ragged_plan(tvc_ctx* ctx, int B, int64_t Lmax, const int64_t* lens, std::vector<RagBatchPlan>* batches, std::vector<int>* gpre, int64_t* S) {
    TVC_CHECK(ragged_split(ctx, ctx->rag_batch_frames, B, Lmax, lens, batches, false));
    gpre->assign((size_t)B, 0);
    int64_t tot = 0;
    for (int b = 0; b < B; ++b) {
        (*gpre)[b] = (int)tot;
        tot += lens[b] / kHop;
        if (tot > 0x7fffffff) return fail(ctx, TVC_ERR_ARG, "ragged encode: more than 2^31 - 1 frames in one call");
    }
    *S = tot;
    return 0;
}

}  // namespace tvc
