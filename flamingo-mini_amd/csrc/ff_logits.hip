// Logits processors of generate(): repetition penalty, no-repeat n-gram ban and minimum length, applied IN PLACE to the rows of logits a
// decode step is about to select from (argmax, ff_sample_token, ff_beam_step).  What transformers' RepetitionPenaltyLogitsProcessor,
// NoRepeatNGramLogitsProcessor and MinLengthLogitsProcessor do with a gather, a where, a scatter, a host loop over the batch and a
// vocabulary-wide mask per step touches at most one entry per history position plus one: here it is one small scatter launch that reads the
// token history and the lengths from device memory, so that it can sit inside the captured decode step.
// One 256-thread workgroup per row.  The row's history (at most FF_LOGITS_HIST_MAX ids) and the ORIGINAL values x[h[j]] are staged in LDS,
// 12 bytes per position; three phases with a barrier between them:
//   0. every thread reads its positions' ids and original values;
//   1. every thread writes f(original): a token that occurs several times is written several times with identical bits, and because every
//      read came before any write it is penalised exactly once - no deduplication;
//   2. the n-gram matches and the eos entry write -inf (after the barrier: bans win over the penalty).
// No reduction and no atomics: equal inputs give equal bits, eager or replayed.  The rules are normative in include/flamingo_fusion.h.
#include <cmath>

#include "ff_common.h"

namespace ff {

template <typename T>
__global__ __launch_bounds__(256) void logits_process_kernel(int V, long long ld, T* __restrict__ logits, const long long* __restrict__ hist, long long hist_ld,
                                                             int hist_cap, const long long* __restrict__ hist_len, float p, float rp, int g, int eos,
                                                             const long long* __restrict__ min_len) {
    extern __shared__ __attribute__((aligned(16))) unsigned char smem_raw[];
    long long* tok = (long long*)smem_raw;                                     // tok[hist_cap] | val[hist_cap]
    float* val = (float*)(smem_raw + (size_t)hist_cap * 8);
    const int tid = threadIdx.x;
    T* x = logits + (long long)blockIdx.x * ld;
    const long long* h = hist + (long long)blockIdx.x * hist_ld;
    const long long len = *hist_len;
    const int n = len < 0 ? 0 : (len > hist_cap ? hist_cap : (int)len);
    const bool penalise = p != 1.f;

    for (int j = tid; j < n; j += 256) {
        const long long t = h[j];
        tok[j] = t;
        if (penalise && t >= 0 && t < V) val[j] = to_f32(x[t]);
    }
    __syncthreads();
    if (penalise) {
        for (int j = tid; j < n; j += 256) {
            const long long t = tok[j];
            if (t < 0 || t >= V) continue;
            const float v = val[j];
            if (v != v) continue;                                               // a NaN keeps its bits
            x[t] = from_f32<T>(v < 0.f ? v * p : v * rp);
        }
        __syncthreads();
    }
    const T ninf = from_f32<T>(-INFINITY);
    if (g >= 1 && n >= g) {
        const int tail = n - g + 1;                                             // the last g - 1 tokens: h[tail .. n - 1]
        for (int i = tid; i <= n - g; i += 256) {
            bool same = true;
            for (int k = 0; k < g - 1 && same; k++) same = tok[i + k] == tok[tail + k];
            const long long t = tok[i + g - 1];
            if (same && t >= 0 && t < V) x[t] = ninf;
        }
    }
    if (tid == 0 && eos >= 0 && min_len != nullptr && n < *min_len) x[eos] = ninf;
}

}  // namespace ff

extern "C" int ff_logits_process(int dtype, int rows, int vocab, long long ld, void* logits, const long long* hist, long long hist_ld, long long hist_cap,
                                 const long long* hist_len, float repetition_penalty, int no_repeat_ngram_size, int eos, const long long* min_len,
                                 ff_stream_t stream) {
    using namespace ff;
    FF_CHECK(logits && hist && hist_len, FF_ERR_SHAPE, "ff_logits_process: null logits, hist or hist_len");
    FF_CHECK(rows > 0 && vocab > 0 && ld >= vocab, FF_ERR_SHAPE, "ff_logits_process: rows %d, vocab %d, ld %lld (need rows > 0, vocab > 0, ld >= vocab)", rows, vocab, ld);
    FF_CHECK(hist_cap >= 1 && hist_ld >= hist_cap, FF_ERR_SHAPE, "ff_logits_process: hist_cap %lld, hist_ld %lld (need hist_cap >= 1, hist_ld >= hist_cap)", hist_cap, hist_ld);
    FF_CHECK(repetition_penalty > 0.f && std::isfinite(repetition_penalty), FF_ERR_SHAPE, "ff_logits_process: repetition_penalty %g must be positive and finite (1 = off)",
             (double)repetition_penalty);
    FF_CHECK(no_repeat_ngram_size >= 0, FF_ERR_SHAPE, "ff_logits_process: no_repeat_ngram_size %d must be >= 0 (0 = off)", no_repeat_ngram_size);
    FF_CHECK(eos >= -1 && eos < vocab, FF_ERR_SHAPE, "ff_logits_process: eos %d outside [-1, vocab %d) (-1 = none)", eos, vocab);
    FF_CHECK(dtype == FF_DTYPE_BF16 || dtype == FF_DTYPE_F32, FF_ERR_UNSUPPORTED, "ff_logits_process: dtype %d", dtype);
    FF_CHECK(hist_cap <= FF_LOGITS_HIST_MAX, FF_ERR_UNSUPPORTED, "ff_logits_process: hist_cap %lld exceeds FF_LOGITS_HIST_MAX %d", hist_cap, FF_LOGITS_HIST_MAX);
    if (repetition_penalty == 1.f && no_repeat_ngram_size == 0 && (eos < 0 || min_len == nullptr)) return FF_OK;      // every processor off: no launch
    const hipStream_t st = (hipStream_t)stream;
    const float rp = 1.0f / repetition_penalty;
    const size_t lds = (size_t)hist_cap * 12;                                  // <= 48 KiB at the cap
    if (dtype == FF_DTYPE_BF16)
        logits_process_kernel<bf16><<<dim3(rows), dim3(256), lds, st>>>(vocab, ld, (bf16*)logits, hist, hist_ld, (int)hist_cap, hist_len, repetition_penalty, rp,
                                                                        no_repeat_ngram_size, eos, min_len);
    else
        logits_process_kernel<float><<<dim3(rows), dim3(256), lds, st>>>(vocab, ld, (float*)logits, hist, hist_ld, (int)hist_cap, hist_len, repetition_penalty, rp,
                                                                         no_repeat_ngram_size, eos, min_len);
    return check_launch("ff_logits_process");
}
