// Real / bogus score on gfx950: forward inference of the layer family the braai VGG6 model uses, on the stamp blocks
// zm_stamps_dev wrote.
//
// Replaces ml_model.predict(make_triplet_for_braai(...)) of the reference's candidate filter (zuds/filterobjects.py:
// 196-240).  The operator is stated in DESIGN.md ("Real / bogus score").
//
//   k_rb_conv<FIRST>  Conv2D 3 x 3 valid stride 1 + bias + relu / linear + the MaxPooling2D that follows (P = 1: none) in one
//                     launch.  One thread per POOLED output pixel and block of RB_COB output channels: the P x P conv outputs
//                     under the pool window are computed one after the other into RB_COB accumulators and folded into a
//                     running maximum, so the un-pooled plane (59 x 59 x 16, 25 x 25 x 32 for VGG6) is never written.
//                     FIRST: the input is the stamp blocks [n][nplanes][S][S] and their float64 norms; each value is divided
//                     by (float)norm as it is read, and channel c reads plane plane_of_channel[c]: no normalised copy.
//                     Weights of a block of output channels lie contiguous per (cin, tap) ([cb][cin][9][RB_COB], re-laid
//                     by zm_rb_model_create, zero-padded to RB_COB): the index is uniform over a wave, so they arrive
//                     through the scalar cache and feed v_fmac as scalar operands - no LDS, no staging.
//   k_rb_pool         a MaxPooling2D that does not follow a convolution
//   k_rb_dense        Dense with >= RB_DENSE_WIDE units: thread = unit, RB_DT triplets per block share every weight read
//   k_rb_dense_small  Dense with fewer units: one wave per (triplet, unit); lane l sums inputs l, l + 64, ... in order,
//                     then an xor tree
//   k_rb_finish       rb[i] = NaN where a norm of the triplet is zero or not finite (the explicit rule), else the score
//
// Arithmetic: fp32 fmaf chains in a fixed order (cin outermost, then ky, kx; bias added last), one thread or one wave per
// output value: no atomics, no dependence on the grid or on the position of a triplet in a batch or chunk.
// Activations live planar ([n][C][H][W]) in two scratch slots of the context ("rb_act_a" / "rb_act_b", ping-pong);
// Flatten's (h, w, c) order is folded into the rows of the Dense kernel that follows it when the model is created.
#include <cmath>

#include "zm_internal.h"

#define RB_COB 8                     // output channels per thread of k_rb_conv (16: 3 x 16 scalar weights spill SGPRs)
#define RB_DT 8                      // triplets per block of k_rb_dense
#define RB_DENSE_WIDE 64             // units from which k_rb_dense is used
#define RB_CH_MAX 64                 // channels of a convolution
#define RB_UNITS_MAX 4096            // units of a Dense layer
#define RB_FLAT_MAX (1 << 20)        // features Flatten may produce

struct rb_src { int nplanes; int poc[ZM_STAMP_PLANES_MAX]; };

__device__ __forceinline__ float rb_act(float v, int act) {
    if (act == ZM_RB_RELU) return v > 0.f ? v : 0.f;             // (NaN -> 0 as v > 0 is false; see k_rb_finish)
    if (act == ZM_RB_SIGMOID) return 1.f / (1.f + expf(-v));
    return v;
}

template <bool FIRST>
__global__ __launch_bounds__(256) void k_rb_conv(const float* __restrict__ in, const double* __restrict__ norms, rb_src src,
                                                 const float* __restrict__ w, const float* __restrict__ bias,
                                                 float* __restrict__ out, int cin, int cout, int H, int W, int P, int OH,
                                                 int OW, int act) {
    const int t = blockIdx.z, cb = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= OH * OW) return;
    const int oy = e / OW, ox = e - oy * OW;
    const float* __restrict__ wb = w + (size_t)cb * cin * 9 * RB_COB;
    const size_t plane = (size_t)H * W;
    float best[RB_COB];
#pragma unroll
    for (int j = 0; j < RB_COB; ++j) best[j] = -INFINITY;
#pragma unroll 1
    for (int dy = 0; dy < P; ++dy) {
#pragma unroll 1
        for (int dx = 0; dx < P; ++dx) {
            const size_t at = (size_t)(oy * P + dy) * W + (ox * P + dx);     // rows .. + 2 < H, columns .. + 2 < W (valid, floor)
            float acc[RB_COB];
#pragma unroll
            for (int j = 0; j < RB_COB; ++j) acc[j] = 0.f;
#pragma unroll 1
            for (int c = 0; c < cin; ++c) {
                const float* __restrict__ ip;
                float nf = 1.f;
                if (FIRST) {
                    const int p = src.poc[c];
                    ip = in + ((size_t)t * src.nplanes + p) * plane + at;
                    nf = (float)norms[(size_t)t * src.nplanes + p];
                } else {
                    ip = in + ((size_t)t * cin + c) * plane + at;
                }
                const float* __restrict__ wk = wb + (size_t)c * 9 * RB_COB;
                // one kernel row at a time: 3 x RB_COB weights are live as scalars, not 9 x RB_COB (with RB_COB = 8: no scalar spills)
#pragma unroll 1
                for (int ky = 0; ky < 3; ++ky) {
                    float v[3];
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx) v[kx] = ip[ky * W + kx];
                    if (FIRST) {
#pragma unroll
                        for (int kx = 0; kx < 3; ++kx) v[kx] = v[kx] / nf;
                    }
#pragma unroll
                    for (int kx = 0; kx < 3; ++kx)
#pragma unroll
                        for (int j = 0; j < RB_COB; ++j) acc[j] = fmaf(v[kx], wk[(ky * 3 + kx) * RB_COB + j], acc[j]);
                }
            }
#pragma unroll
            for (int j = 0; j < RB_COB; ++j) {
                const int co = cb * RB_COB + j;
                const float r = rb_act(acc[j] + (co < cout ? bias[co] : 0.f), act);
                best[j] = fmaxf(best[j], r);
            }
        }
    }
#pragma unroll
    for (int j = 0; j < RB_COB; ++j) {
        const int co = cb * RB_COB + j;
        if (co < cout) out[(((size_t)t * cout + co) * OH + oy) * OW + ox] = best[j];
    }
}

__global__ __launch_bounds__(256) void k_rb_pool(const float* __restrict__ in, float* __restrict__ out, int C, int H, int W,
                                                 int P, int OH, int OW) {
    const int t = blockIdx.z, c = blockIdx.y;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= OH * OW) return;
    const int oy = e / OW, ox = e - oy * OW;
    const float* ip = in + ((size_t)t * C + c) * H * W + (size_t)(oy * P) * W + ox * P;
    float best = -INFINITY;
    for (int dy = 0; dy < P; ++dy)
        for (int dx = 0; dx < P; ++dx) best = fmaxf(best, ip[dy * W + dx]);
    out[(((size_t)t * C + c) * OH + oy) * OW + ox] = best;
}

__global__ __launch_bounds__(256) void k_rb_dense(const float* __restrict__ x, const float* __restrict__ w,
                                                  const float* __restrict__ bias, float* __restrict__ y, int n, int nin,
                                                  int nout, int act) {
    const int j = blockIdx.x * 256 + threadIdx.x;
    const int t0 = blockIdx.y * RB_DT;
    if (j >= nout) return;
    const float* xt[RB_DT];
#pragma unroll
    for (int t = 0; t < RB_DT; ++t) xt[t] = x + (size_t)min(t0 + t, n - 1) * nin;      // (a tail block re-reads the last triplet)
    float acc[RB_DT];
#pragma unroll
    for (int t = 0; t < RB_DT; ++t) acc[t] = 0.f;
#pragma unroll 4
    for (int i = 0; i < nin; ++i) {
        const float wv = w[(size_t)i * nout + j];
#pragma unroll
        for (int t = 0; t < RB_DT; ++t) acc[t] = fmaf(xt[t][i], wv, acc[t]);
    }
    const float b = bias[j];
#pragma unroll
    for (int t = 0; t < RB_DT; ++t)
        if (t0 + t < n) y[(size_t)(t0 + t) * nout + j] = rb_act(acc[t] + b, act);
}

__global__ __launch_bounds__(64) void k_rb_dense_small(const float* __restrict__ x, const float* __restrict__ w,
                                                       const float* __restrict__ bias, float* __restrict__ y, int nin,
                                                       int nout, int act) {
    const int j = blockIdx.x, t = blockIdx.y, lane = threadIdx.x;
    const float* xt = x + (size_t)t * nin;
    float s = 0.f;
    for (int i = lane; i < nin; i += 64) s = fmaf(xt[i], w[(size_t)i * nout + j], s);
#pragma unroll
    for (int of = 32; of >= 1; of >>= 1) s += __shfl_xor(s, of);
    if (lane == 0) y[(size_t)t * nout + j] = rb_act(s + bias[j], act);
}

__global__ __launch_bounds__(256) void k_rb_finish(const float* __restrict__ score, const double* __restrict__ norms,
                                                   rb_src src, int cin, int n, float* __restrict__ rb) {
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= n) return;
    bool bad = false;
    for (int c = 0; c < cin; ++c) {
        const double v = norms[(size_t)t * src.nplanes + src.poc[c]];
        bad = bad || !(fabs(v) <= 1.7976931348623157e308) || v == 0.0;     // NaN, +-inf, zero
    }
    rb[t] = bad ? __builtin_nanf("") : score[t];
}

// ---- host ----------------------------------------------------------------------------------------------------------
enum { RB_STEP_CONV = 1, RB_STEP_POOL = 2, RB_STEP_DENSE = 3 };
struct rb_step {
    int kind, act;
    int cin, cout, H, W, P, OH, OW;      // conv / pool (pool: cin = cout = channels); dense: cin = inputs, cout = units
    size_t w_off, b_off;                 // in the device blob (floats)
    size_t out_floats;                   // per triplet
};
struct zm_rb_model {
    int device = 0, in_size = 0, in_channels = 0;
    std::vector<rb_step> steps;
    float* blob = nullptr;
    size_t act_floats[2] = {0, 0};       // per triplet: outputs of the even / odd steps (ping-pong)
};

static const char* rb_type_name(int t) {
    return t == ZM_RB_CONV2D ? "Conv2D" : t == ZM_RB_MAXPOOL ? "MaxPooling2D" : t == ZM_RB_FLATTEN ? "Flatten"
         : t == ZM_RB_DENSE ? "Dense" : "unknown";
}

extern "C" int zm_rb_model_create(zm_ctx* ctx, int in_size, int in_channels, int nlayers, const zm_rb_layer* layers,
                                  const float* weights, int64_t nweights, zm_rb_model** out) {
    ZM_CHECK(ctx && layers && weights && out, "zm_rb_model_create: null argument");
    ZM_CHECK(nlayers >= 1 && nlayers <= 64, "zm_rb_model_create: 1 .. 64 layers (got %d)", nlayers);
    ZM_CHECK(in_size >= 3 && in_size <= ZM_STAMP_MAX, "zm_rb_model_create: input size must be 3 .. %d (got %d)", ZM_STAMP_MAX, in_size);
    ZM_CHECK(in_channels >= 1 && in_channels <= ZM_STAMP_PLANES_MAX, "zm_rb_model_create: 1 .. %d input channels (got %d)",
             ZM_STAMP_PLANES_MAX, in_channels);
    ZM_CHECK(nweights >= 1, "zm_rb_model_create: no weights");
    ZM_CHECK(layers[0].type == ZM_RB_CONV2D, "zm_rb_model_create: the first layer must be Conv2D (it reads the stamps); got %s",
             rb_type_name(layers[0].type));
    std::vector<rb_step> steps;
    std::vector<float> blob;
    int C = in_channels, H = in_size, W = in_size;
    long long flat = 0;                   // > 0: the tensor is a vector of that many features
    bool flat_hwc = false;                // ... that Flatten made of a C x H x W tensor (the next Dense permutes its rows)
    int fC = 0, fH = 0, fW = 0;
    auto span_ok = [&](int64_t off, long long count) { return off >= 0 && count >= 0 && off <= nweights && count <= nweights - off; };
    for (int l = 0; l < nlayers; ++l) {
        const zm_rb_layer& L = layers[l];
        if (L.type == ZM_RB_CONV2D) {
            ZM_CHECK(flat == 0, "zm_rb_model_create: layer %d: Conv2D behind Flatten", l);
            ZM_CHECK(L.ksize == 3, "zm_rb_model_create: layer %d: only 3 x 3 kernels (got %d)", l, L.ksize);
            ZM_CHECK(L.stride == 1, "zm_rb_model_create: layer %d: only stride 1 (got %d)", l, L.stride);
            ZM_CHECK(L.padding == ZM_RB_VALID, "zm_rb_model_create: layer %d: only 'valid' padding", l);
            ZM_CHECK(L.activation == ZM_RB_LINEAR || L.activation == ZM_RB_RELU,
                     "zm_rb_model_create: layer %d: Conv2D takes relu or linear (got %d)", l, L.activation);
            ZM_CHECK(L.cin == C, "zm_rb_model_create: layer %d: %d input channels, the tensor has %d", l, L.cin, C);
            ZM_CHECK(L.cout >= 1 && L.cout <= RB_CH_MAX, "zm_rb_model_create: layer %d: 1 .. %d output channels (got %d)", l,
                     RB_CH_MAX, L.cout);
            ZM_CHECK(L.cin <= RB_CH_MAX, "zm_rb_model_create: layer %d: at most %d input channels (got %d)", l, RB_CH_MAX, L.cin);
            ZM_CHECK(H >= 3 && W >= 3, "zm_rb_model_create: layer %d: a %d x %d tensor is smaller than the kernel", l, H, W);
            ZM_CHECK(span_ok(L.w_off, 9LL * L.cin * L.cout) && span_ok(L.b_off, L.cout),
                     "zm_rb_model_create: layer %d: weights lie outside the blob of %lld floats", l, (long long)nweights);
            rb_step s{};
            s.kind = RB_STEP_CONV;
            s.act = L.activation;
            s.cin = L.cin; s.cout = L.cout; s.H = H; s.W = W; s.P = 1; s.OH = H - 2; s.OW = W - 2;
            const int ncb = zm_div_up(L.cout, RB_COB);
            s.w_off = blob.size();
            blob.resize(blob.size() + (size_t)ncb * L.cin * 9 * RB_COB, 0.f);
            // Keras [kh][kw][cin][cout] -> [cb][cin][tap][RB_COB]
            for (int k = 0; k < 9; ++k)
                for (int c = 0; c < L.cin; ++c)
                    for (int co = 0; co < L.cout; ++co)
                        blob[s.w_off + (((size_t)(co / RB_COB) * L.cin + c) * 9 + k) * RB_COB + co % RB_COB] =
                            weights[L.w_off + ((size_t)k * L.cin + c) * L.cout + co];
            s.b_off = blob.size();
            blob.insert(blob.end(), weights + L.b_off, weights + L.b_off + L.cout);
            C = L.cout; H = s.OH; W = s.OW;
            steps.push_back(s);
        } else if (L.type == ZM_RB_MAXPOOL) {
            ZM_CHECK(flat == 0, "zm_rb_model_create: layer %d: MaxPooling2D behind Flatten", l);
            ZM_CHECK(L.pool >= 1 && L.pool <= 16, "zm_rb_model_create: layer %d: pool size 1 .. 16 (got %d)", l, L.pool);
            ZM_CHECK(L.stride == L.pool, "zm_rb_model_create: layer %d: the pool's stride must equal its size (%d, %d)", l,
                     L.stride, L.pool);
            ZM_CHECK(L.padding == ZM_RB_VALID, "zm_rb_model_create: layer %d: only 'valid' padding", l);
            ZM_CHECK(H / L.pool >= 1 && W / L.pool >= 1, "zm_rb_model_create: layer %d: pool %d of a %d x %d tensor", l, L.pool, H, W);
            if (!steps.empty() && steps.back().kind == RB_STEP_CONV && steps.back().P == 1 && layers[l - 1].type == ZM_RB_CONV2D) {
                rb_step& s = steps.back();                 // fused into the convolution's epilogue
                s.P = L.pool;
                s.OH = H / L.pool; s.OW = W / L.pool;
            } else {
                rb_step s{};
                s.kind = RB_STEP_POOL;
                s.cin = s.cout = C; s.H = H; s.W = W; s.P = L.pool; s.OH = H / L.pool; s.OW = W / L.pool;
                steps.push_back(s);
            }
            H /= L.pool; W /= L.pool;
        } else if (L.type == ZM_RB_FLATTEN) {
            ZM_CHECK(flat == 0, "zm_rb_model_create: layer %d: Flatten of a vector", l);
            flat = (long long)C * H * W;
            ZM_CHECK(flat <= RB_FLAT_MAX, "zm_rb_model_create: layer %d: %lld features (at most %d)", l, flat, RB_FLAT_MAX);
            flat_hwc = true;
            fC = C; fH = H; fW = W;
        } else if (L.type == ZM_RB_DENSE) {
            ZM_CHECK(flat > 0, "zm_rb_model_create: layer %d: Dense needs a Flatten before it", l);
            ZM_CHECK(L.activation == ZM_RB_LINEAR || L.activation == ZM_RB_RELU || L.activation == ZM_RB_SIGMOID,
                     "zm_rb_model_create: layer %d: Dense takes relu, sigmoid or linear (got %d)", l, L.activation);
            ZM_CHECK(L.cin == flat, "zm_rb_model_create: layer %d: %d inputs, the tensor has %lld", l, L.cin, flat);
            ZM_CHECK(L.cout >= 1 && L.cout <= RB_UNITS_MAX, "zm_rb_model_create: layer %d: 1 .. %d units (got %d)", l, RB_UNITS_MAX, L.cout);
            ZM_CHECK(span_ok(L.w_off, (long long)L.cin * L.cout) && span_ok(L.b_off, L.cout),
                     "zm_rb_model_create: layer %d: weights lie outside the blob of %lld floats", l, (long long)nweights);
            rb_step s{};
            s.kind = RB_STEP_DENSE;
            s.act = L.activation;
            s.cin = L.cin; s.cout = L.cout;
            s.w_off = blob.size();
            blob.resize(blob.size() + (size_t)L.cin * L.cout);
            for (long long i = 0; i < flat; ++i) {
                long long src = i;                         // row of the Keras kernel that input i of OUR layout multiplies
                if (flat_hwc) {                            // ours: (c, h, w); Keras: (h, w, c)
                    const long long c = i / ((long long)fH * fW), hw = i - c * fH * fW;
                    src = hw * fC + c;
                }
                memcpy(&blob[s.w_off + (size_t)i * L.cout], weights + L.w_off + (size_t)src * L.cout, sizeof(float) * L.cout);
            }
            s.b_off = blob.size();
            blob.insert(blob.end(), weights + L.b_off, weights + L.b_off + L.cout);
            flat = L.cout;
            flat_hwc = false;
            steps.push_back(s);
        } else {
            ZM_CHECK(false, "zm_rb_model_create: layer %d: unsupported layer type %d (Conv2D, MaxPooling2D, Flatten, Dense)", l, L.type);
        }
    }
    ZM_CHECK(flat == 1 && steps.back().kind == RB_STEP_DENSE, "zm_rb_model_create: the model must end in a Dense layer of one unit");
    zm_rb_model* m = new zm_rb_model();
    m->device = ctx->device;
    m->in_size = in_size;
    m->in_channels = in_channels;
    for (size_t i = 0; i < steps.size(); ++i) {
        rb_step& s = steps[i];
        s.out_floats = s.kind == RB_STEP_DENSE ? (size_t)s.cout : (size_t)s.cout * s.OH * s.OW;
        m->act_floats[i & 1] = std::max(m->act_floats[i & 1], s.out_floats);
    }
    m->steps = steps;
    if (hipSetDevice(ctx->device) != hipSuccess || hipMalloc((void**)&m->blob, blob.size() * sizeof(float)) != hipSuccess ||
        hipMemcpy(m->blob, blob.data(), blob.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
        if (m->blob) (void)hipFree(m->blob);
        delete m;
        zm_set_error("zm_rb_model_create: could not upload %zu floats", blob.size());
        return 1;
    }
    *out = m;
    return 0;
}

extern "C" int zm_rb_model_destroy(zm_rb_model* model) {
    if (!model) return 0;
    (void)hipSetDevice(model->device);
    if (model->blob) (void)hipFree(model->blob);           // (waits for work that still reads it)
    delete model;
    return 0;
}

static int rb_check(const char* who, zm_ctx* ctx, const zm_rb_model* m, int n, const float* blocks, const double* norms,
                    int nplanes, const int32_t* poc, const float* rb, rb_src* src) {
    ZM_CHECK(ctx && m && poc, "%s: null argument", who);
    ZM_CHECK(n >= 0, "%s: n must not be negative (got %d)", who, n);
    ZM_CHECK(n == 0 || (blocks && norms && rb), "%s: null argument", who);
    ZM_CHECK(ctx->device == m->device, "%s: the model lives on device %d, the context on %d", who, m->device, ctx->device);
    ZM_CHECK(nplanes >= 1 && nplanes <= ZM_STAMP_PLANES_MAX, "%s: 1 .. %d planes (got %d)", who, ZM_STAMP_PLANES_MAX, nplanes);
    memset(src, 0, sizeof(*src));
    src->nplanes = nplanes;
    for (int c = 0; c < m->in_channels; ++c) {
        ZM_CHECK(poc[c] >= 0 && poc[c] < nplanes, "%s: plane_of_channel[%d] = %d is not one of the %d planes", who, c, poc[c], nplanes);
        src->poc[c] = poc[c];
    }
    return 0;
}

extern "C" int zm_rb_score_dev(zm_ctx* ctx, const zm_rb_model* m, int n, const float* blocks_dev, const double* norms_dev,
                               int nplanes, const int32_t* plane_of_channel, float* rb_dev) {
    rb_src src;
    ZM_TRY(rb_check("zm_rb_score_dev", ctx, m, n, blocks_dev, norms_dev, nplanes, plane_of_channel, rb_dev, &src));
    if (n == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const int cap = std::min(n, ZM_RB_CHUNK);
    float* buf[2] = {nullptr, nullptr};
    ZM_TRY(ctx->get("rb_act_a", sizeof(float) * m->act_floats[0] * cap, (void**)&buf[0]));
    ZM_TRY(ctx->get("rb_act_b", sizeof(float) * std::max<size_t>(m->act_floats[1], 1) * cap, (void**)&buf[1]));
    const size_t S2 = (size_t)m->in_size * m->in_size;
    zm_scope_timer timer(ctx, "rb_score");
    for (int c0 = 0; c0 < n; c0 += ZM_RB_CHUNK) {
        const int nc = std::min(ZM_RB_CHUNK, n - c0);
        const float* blocks = blocks_dev + (size_t)c0 * nplanes * S2;
        const double* norms = norms_dev + (size_t)c0 * nplanes;
        const float* cur = nullptr;
        for (size_t i = 0; i < m->steps.size(); ++i) {
            const rb_step& s = m->steps[i];
            float* dst = buf[i & 1];
            if (s.kind == RB_STEP_CONV) {
                const dim3 grid((unsigned)zm_div_up(s.OH * s.OW, 256), (unsigned)zm_div_up(s.cout, RB_COB), (unsigned)nc);
                if (i == 0)
                    hipLaunchKernelGGL(k_rb_conv<true>, grid, dim3(256), 0, ctx->stream, blocks, norms, src, m->blob + s.w_off,
                                       m->blob + s.b_off, dst, s.cin, s.cout, s.H, s.W, s.P, s.OH, s.OW, s.act);
                else
                    hipLaunchKernelGGL(k_rb_conv<false>, grid, dim3(256), 0, ctx->stream, cur, (const double*)nullptr, src,
                                       m->blob + s.w_off, m->blob + s.b_off, dst, s.cin, s.cout, s.H, s.W, s.P, s.OH, s.OW, s.act);
            } else if (s.kind == RB_STEP_POOL) {
                const dim3 grid((unsigned)zm_div_up(s.OH * s.OW, 256), (unsigned)s.cout, (unsigned)nc);
                hipLaunchKernelGGL(k_rb_pool, grid, dim3(256), 0, ctx->stream, cur, dst, s.cout, s.H, s.W, s.P, s.OH, s.OW);
            } else if (s.cout >= RB_DENSE_WIDE) {
                const dim3 grid((unsigned)zm_div_up(s.cout, 256), (unsigned)zm_div_up(nc, RB_DT));
                hipLaunchKernelGGL(k_rb_dense, grid, dim3(256), 0, ctx->stream, cur, m->blob + s.w_off, m->blob + s.b_off, dst, nc,
                                   s.cin, s.cout, s.act);
            } else {
                hipLaunchKernelGGL(k_rb_dense_small, dim3((unsigned)s.cout, (unsigned)nc), dim3(64), 0, ctx->stream, cur,
                                   m->blob + s.w_off, m->blob + s.b_off, dst, s.cin, s.cout, s.act);
            }
            ZM_HIP(hipGetLastError());
            cur = dst;
        }
        hipLaunchKernelGGL(k_rb_finish, dim3((unsigned)zm_div_up(nc, 256)), dim3(256), 0, ctx->stream, cur, norms, src,
                           m->in_channels, nc, rb_dev + c0);
        ZM_HIP(hipGetLastError());
    }
    return 0;
}

extern "C" int zm_rb_score(zm_ctx* ctx, const zm_rb_model* m, int n, const float* blocks, const double* norms, int nplanes,
                           const int32_t* plane_of_channel, float* rb) {
    rb_src src;
    ZM_TRY(rb_check("zm_rb_score", ctx, m, n, blocks, norms, nplanes, plane_of_channel, rb, &src));
    if (n == 0) return 0;
    ZM_HIP(hipSetDevice(ctx->device));
    const size_t bb = (((size_t)n * nplanes * m->in_size * m->in_size * 4) + 15) & ~(size_t)15;
    const size_t nb = (((size_t)n * nplanes * 8) + 15) & ~(size_t)15, rbb = (size_t)n * 4;
    char* d = nullptr;
    ZM_TRY(ctx->get("h_rb_io", bb + nb + rbb, (void**)&d));
    ZM_HIP(hipMemcpyAsync(d, blocks, (size_t)n * nplanes * m->in_size * m->in_size * 4, hipMemcpyHostToDevice, ctx->stream));
    ZM_HIP(hipMemcpyAsync(d + bb, norms, (size_t)n * nplanes * 8, hipMemcpyHostToDevice, ctx->stream));
    ZM_TRY(zm_rb_score_dev(ctx, m, n, (const float*)d, (const double*)(d + bb), nplanes, plane_of_channel, (float*)(d + bb + nb)));
    ZM_HIP(hipMemcpyAsync(rb, d + bb + nb, rbb, hipMemcpyDeviceToHost, ctx->stream));
    ZM_HIP(hipStreamSynchronize(ctx->stream));
    return 0;
}
