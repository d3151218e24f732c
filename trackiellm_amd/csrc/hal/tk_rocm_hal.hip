/*
 * tk_rocm_hal.hip — dispatcher + kernel launchers of the reference's ROCm HAL surface
 * (src/gpu/rocm/tk_rocm_dispatch.hpp:83-217, src/gpu/rocm/tk_rocm_kernels.hpp:96,133,176).
 */
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdlib.h>

#include <vector>

#include "../common/tk_exact_math.h"
#include "../common/tk_lang_pick.h"
#include "tk/tk_mi355x_ext.h"

#include "../vision/tk_vision_engine.h"
#include "../vision/tk_depth_engine.h"
#include "../audio/tk_audio_engine.h"
#include "tk/tk_rocm_hal.h"
#include "../nn/tk_gemm_tiled.h"
#include "../nn/tk_nn_kernels.h"
#include "../llm/tk_llm_kernels.h"

struct tk_gpu_buffer_s {
    void* dptr;
    size_t size;
};

struct tk_rocm_dispatcher_s {
    int device;
    hipStream_t compute, h2d, d2h; /* three non-blocking streams, as the reference dispatcher */
    hipEvent_t ev_upload, ev_compute;
};

/* out = raw * scale + shift  (src/gpu/rocm/tk_rocm_kernels.cpp:148-163), grid-stride, float4-free: the maps are tiny */
__global__ void k_postprocess_depth(tk_postprocess_depth_params_t p) {
    const size_t n = (size_t)p.width * p.height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x)
        p.d_metric_depth_map[i] = p.d_raw_depth_map[i] * p.scale + p.shift;
}

/* pinhole unprojection (src/gpu/rocm/tk_rocm_kernels.cpp:176-202): depth <= 0 -> origin */
__global__ void k_depth_to_points(tk_depth_to_points_params_t p) {
    const size_t n = (size_t)p.width * p.height;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
        const float d = p.d_metric_depth_map[i];
        tk_float3 o = {0.0f, 0.0f, 0.0f};
        if (d > 0.0f) {
            const float u = (float)(i % p.width), v = (float)(i / p.width);
            o.x = tk_divf((u - p.cx) * d, p.fx);
            o.y = tk_divf((v - p.cy) * d, p.fy);
            o.z = d;
        }
        p.d_point_cloud[i] = o;
    }
}

/* multiply-by-scale variant of the canonical pre-processor for scale != 1/255 */
__global__ void k_preprocess_scaled(TkPreprocessArgs a, float scale) {
    const uint32_t ox = blockIdx.x * blockDim.x + threadIdx.x, oy = blockIdx.y * blockDim.y + threadIdx.y;
    if (ox >= a.out_w || oy >= a.out_h) return;
    const float x_ratio = tk_divf((float)a.in_w - 1.0f, (float)a.out_w), y_ratio = tk_divf((float)a.in_h - 1.0f, (float)a.out_h);
    const float gx = x_ratio * (float)ox, gy = y_ratio * (float)oy;
    const int x = (int)gx, y = (int)gy;
    const float xd = gx - (float)x, yd = gy - (float)y;
    const int x1 = x + 1 < (int)a.in_w ? x + 1 : x, y1 = y + 1 < (int)a.in_h ? y + 1 : y;
    const uint8_t* r0 = a.src + (size_t)y * a.in_stride;
    const uint8_t* r1 = a.src + (size_t)y1 * a.in_stride;
    const size_t np = (size_t)a.out_w * a.out_h, pix = (size_t)oy * a.out_w + ox;
    for (int c = 0; c < 3; ++c) {
        float v = ((float)r0[x * a.bpp + c] * (1.0f - xd)) * (1.0f - yd);
        v = v + ((float)r0[x1 * a.bpp + c] * xd) * (1.0f - yd);
        v = v + ((float)r1[x * a.bpp + c] * (1.0f - xd)) * yd;
        v = v + ((float)r1[x1 * a.bpp + c] * xd) * yd;
        const float o = tk_divf(v * scale - a.mean[c], a.std_dev[c]);
        if (a.nhwc) a.dst[pix * 3 + c] = o;
        else a.dst[c * np + pix] = o;
    }
}

/* the pre-processor for a given scale: 1/255 (or 0, "unset") is the canonical kernel's own division by 255, any other value the multiply-by-scale
 * variant.  Returns the choice: 0 k_preprocess, 1 k_preprocess_scaled; with dry, the choice alone */
static int launch_preprocess_for_scale(const TkPreprocessArgs& a, float scale, hipStream_t s, bool dry) {
    if (scale == 1.0f / 255.0f || scale == 0.0f) {
        if (!dry) tk_launch_preprocess(a, s);
        return 0;
    }
    if (!dry) hipLaunchKernelGGL(k_preprocess_scaled, dim3((a.out_w + 63) / 64, (a.out_h + 3) / 4), dim3(64, 4), 0, s, a, scale);
    return 1;
}

/* the two element-wise depth kernels' grid: one thread per element up to TK_DEPTH_GRID_CAP blocks of 256, a grid-stride loop beyond */
#define TK_DEPTH_GRID_CAP 2048
static unsigned depth_grid_blocks(size_t n) {
    const size_t blocks = (n + 255) / 256;
    return (unsigned)(blocks > TK_DEPTH_GRID_CAP ? TK_DEPTH_GRID_CAP : blocks);
}

static tk_error_code_t launch_status() { return hipGetLastError() == hipSuccess ? TK_SUCCESS : TK_ERROR_GPU_KERNEL_LAUNCH; }

extern "C" {

tk_error_code_t tk_kernels_preprocess_image(const tk_preprocess_params_t* p, tk_hip_stream_t stream) {
    if (!p || !p->d_input_image || !p->d_output_tensor || p->output_width == 0 || p->output_height == 0) return TK_ERROR_INVALID_ARGUMENT;
    if (p->input_width < 2 || p->input_height < 2 || p->input_stride_bytes < p->input_width * 3) return TK_ERROR_INVALID_ARGUMENT;
    TkPreprocessArgs a{};
    a.src = p->d_input_image; a.in_w = p->input_width; a.in_h = p->input_height; a.in_stride = p->input_stride_bytes; a.bpp = 3;
    a.dst = p->d_output_tensor; a.out_w = p->output_width; a.out_h = p->output_height; a.nhwc = 0;
    a.mean[0] = p->mean.x; a.mean[1] = p->mean.y; a.mean[2] = p->mean.z;
    a.std_dev[0] = p->std_dev.x; a.std_dev[1] = p->std_dev.y; a.std_dev[2] = p->std_dev.z;
    (void)launch_preprocess_for_scale(a, p->scale, (hipStream_t)stream, false);
    return launch_status();
}

tk_error_code_t tk_kernels_preprocess_image_generic(const tk_preprocess_params_generic_t* g, tk_hip_stream_t stream) {
    if (!g) return TK_ERROR_INVALID_ARGUMENT;
    tk_preprocess_params_t p;
    p.d_input_image = (const unsigned char*)g->d_input_image; p.input_width = g->input_width; p.input_height = g->input_height;
    p.input_stride_bytes = g->input_stride_bytes; p.d_output_tensor = (float*)g->d_output_tensor; p.output_width = g->output_width;
    p.output_height = g->output_height; p.mean = tk_float3{g->mean.x, g->mean.y, g->mean.z}; p.std_dev = tk_float3{g->std_dev.x, g->std_dev.y, g->std_dev.z};
    p.scale = 1.0f / 255.0f;
    return tk_kernels_preprocess_image(&p, stream);
}

tk_error_code_t tk_kernels_postprocess_depth_map(const tk_postprocess_depth_params_t* p, tk_hip_stream_t stream) {
    if (!p || !p->d_raw_depth_map || !p->d_metric_depth_map || p->width == 0 || p->height == 0) return TK_ERROR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(k_postprocess_depth, dim3(depth_grid_blocks((size_t)p->width * p->height)), dim3(256), 0, (hipStream_t)stream, *p);
    return launch_status();
}

tk_error_code_t tk_kernels_softmax(const tk_softmax_params_t* p, tk_hip_stream_t stream) {
    if (!p || !p->d_input_tensor || !p->d_output_tensor || p->num_rows == 0 || p->num_cols == 0 || p->num_rows > 0x7fffffffu || p->num_cols > 0x7fffffffu)
        return TK_ERROR_INVALID_ARGUMENT;
    if (p->d_output_tensor != p->d_input_tensor &&
        hipMemcpyAsync(p->d_output_tensor, p->d_input_tensor, (size_t)p->num_rows * p->num_cols * sizeof(float), hipMemcpyDeviceToDevice,
                       (hipStream_t)stream) != hipSuccess)
        return TK_ERROR_GPU_ROCM_ERROR;
    if (!tk_launch_softmax_rows((float*)p->d_output_tensor, (int)p->num_rows, (int)p->num_cols, (int)p->num_cols, (hipStream_t)stream))
        return TK_ERROR_INVALID_ARGUMENT;
    return launch_status();
}

tk_error_code_t tk_mi355x_gemm_pair(int device, int M, int N, int K, const float* a, const float* w, const float* bias, const float* residual, int act,
                                    int f16, float* c_staged, float* c_tiled) {
    if (M <= 0 || N <= 0 || K <= 0 || K % 128 || !a || !w || !c_staged || !c_tiled || act < 0 || act > 3) return TK_ERROR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    if (!tk_nn_prepare_device() || !tk_gemm_tiled_prepare_device()) return TK_ERROR_GPU_ROCM_ERROR;
    const size_t na = (size_t)M * K, nw = (size_t)N * K, nc = (size_t)M * N;
    const int64_t blk = M >= 256 ? 256 : (M > 128 ? 256 : M > 64 ? 128 : M > 32 ? 64 : M > 16 ? 32 : 16);
    const size_t nimg = (size_t)(((int64_t)M + blk - 1) / blk * blk) * K;
    float *da = nullptr, *dw = nullptr, *db = nullptr, *dr = nullptr, *dc = nullptr, *dimg = nullptr;
    uint16_t* dwh = nullptr;
    uint8_t* dt = nullptr;
    bool ok = hipMalloc((void**)&da, na * 4) == hipSuccess && hipMalloc((void**)&dw, nw * 4) == hipSuccess && hipMalloc((void**)&dc, nc * 4) == hipSuccess &&
              hipMalloc((void**)&dimg, nimg * 4) == hipSuccess && hipMalloc((void**)&dt, tk_tiled_weight_bytes(N, K, f16 ? 2 : 4)) == hipSuccess &&
              (!bias || hipMalloc((void**)&db, (size_t)N * 4) == hipSuccess) && (!residual || hipMalloc((void**)&dr, nc * 4) == hipSuccess) &&
              (!f16 || hipMalloc((void**)&dwh, nw * 2) == hipSuccess);
    ok = ok && hipMemcpy(da, a, na * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dw, w, nw * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!bias || hipMemcpy(db, bias, (size_t)N * 4, hipMemcpyHostToDevice) == hipSuccess) &&
         (!residual || hipMemcpy(dr, residual, nc * 4, hipMemcpyHostToDevice) == hipSuccess) && hipMemset(dimg, 0, nimg * 4) == hipSuccess;
    if (ok) {
        std::vector<uint16_t> wh;
        if (f16) { /* the f16 checkpoint's weights; the staged kernel reads the same values through its f16 B operand */
            wh.resize(nw);
            for (size_t i = 0; i < nw; ++i) wh[i] = tk_f32_to_f16(w[i]);
            ok = hipMemcpy(dwh, wh.data(), nw * 2, hipMemcpyHostToDevice) == hipSuccess;
        }
        /* staged kernel: with f16 the activations must already be f16-rounded values, as the LLM's producers write them */
        std::vector<float> ar;
        if (ok && f16) {
            ar.resize(na);
            for (size_t i = 0; i < na; ++i) ar[i] = tk_f16_to_f32(tk_f32_to_f16(a[i]));
            ok = hipMemcpy(da, ar.data(), na * 4, hipMemcpyHostToDevice) == hipSuccess;
        }
        if (ok) {
            TkGemm g{};
            g.A = da; g.B = f16 ? (const float*)dwh : dw; g.C = dc; g.bias = db; g.residual = dr;
            g.M = M; g.N = N; g.K = K; g.lda = K; g.ldb = K; g.ldc = N; g.ldr = N; g.act = act; g.alpha = 1.0f; g.batch = 1; g.b_f16 = f16 ? 1 : 0;
            tk_launch_gemm(g, nullptr);
            ok = hipMemcpy(c_staged, dc, nc * 4, hipMemcpyDeviceToHost) == hipSuccess && hipMemset(dc, 0, nc * 4) == hipSuccess;
        }
        if (ok) {
            tk_launch_tile_weights(f16 ? (const void*)dwh : (const void*)dw, f16 ? 2 : 4, N, K, dt, nullptr);
            tk_launch_pack_a(da, M, K, K, 0, dimg, nullptr); /* da already holds the f16-rounded values in the f16 case */
            TkTiledGemm t{};
            t.tiles[0] = dt; t.row_tiles[0] = (N + 15) / 16; t.nseg = 1; t.wbytes = f16 ? 2 : 4;
            t.K = K; t.ks = 1; t.ldc = N; t.n_valid = N; t.nrows = M; t.a_img = dimg; t.a_ts = (size_t)K * 16; t.out = dc;
            t.bias = db; t.residual = dr; t.ldr = N; t.act = act; t.add_zero_bias = 1;
            ok = tk_launch_gemm_tiled(t, nullptr) && hipGetLastError() == hipSuccess && hipMemcpy(c_tiled, dc, nc * 4, hipMemcpyDeviceToHost) == hipSuccess;
        }
    }
    void* ptrs[] = {da, dw, db, dr, dc, dimg, dwh, dt};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    return ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
}

/* the highest element index each operand of a launch can touch (-1: never read), from the loaders' own predicates: a row m < M, a column
 * k < K / n < N, every batch member; false: a field outside what a launch may hold.  Extents are capped so that no product leaves int64. */
struct ProbeReach { int64_t a, b, c, r; };
static bool probe_reach(const tk_mi355x_gemm_probe_t& p, ProbeReach& o) {
    const int64_t cap = (int64_t)1 << 28;
    auto dim = [&](int64_t v) { return v >= 1 && v <= cap; };
    auto str = [&](int64_t v) { return v >= 0 && v <= cap; };
    if (!dim(p.M) || !dim(p.N) || !dim(p.K) || !dim(p.ldb) || !dim(p.ldc) || p.ldc < p.N || p.act < 0 || p.act > 3) return false;
    if (p.batch < 1 || p.batch > 4096 || p.batch_inner < 0 || p.batch_inner > p.batch || (p.batch_inner > 0 && p.batch % p.batch_inner)) return false;
    if ((p.b_kn != 0 && p.b_kn != 1) || (p.b_f16 != 0 && p.b_f16 != 1) || p.a_offset < 0 || p.a_offset > 64 || p.b_offset < 0 || p.b_offset > 64) return false;
    const int64_t st[8] = {p.sA, p.sB, p.sC, p.sR, p.sA2, p.sB2, p.sC2, p.sR2};
    for (int64_t v : st) if (!str(v)) return false;
    if (p.residual && (!dim(p.ldr) || p.ldr < p.N)) return false;
    /* offset of the last batch member along one operand's strides */
    const int64_t zi = p.batch_inner > 0 ? p.batch_inner - 1 : p.batch - 1, zo = p.batch_inner > 0 ? p.batch / p.batch_inner - 1 : 0;
    auto last = [&](int64_t s1, int64_t s2) { return zi * s1 + (p.batch_inner > 0 ? zo * s2 : 0); };
    if (p.im_C > 0) {
        if (!dim(p.im_H) || !dim(p.im_W) || !dim(p.im_ldx) || p.im_ldx < p.im_C || !dim(p.im_kw) || !dim(p.im_stride) || p.im_pad < 0 || p.im_pad > cap ||
            !dim(p.im_Ho) || !dim(p.im_Wo) || p.batch != 1 || p.K % ((int64_t)p.im_C * p.im_kw))
            return false;
        const int64_t images = ((int64_t)p.M - 1) / ((int64_t)p.im_Ho * p.im_Wo) + 1; /* a row addresses image m / (Ho Wo), any pixel inside it */
        if (images > cap / p.im_H / p.im_W) return false;
        o.a = (images * p.im_H * p.im_W - 1) * p.im_ldx + p.im_C - 1;
    } else {
        if (p.im_C < 0 || !dim(p.lda)) return false;
        o.a = last(p.sA, p.sA2) + ((int64_t)p.M - 1) * p.lda + p.K - 1;
    }
    o.b = last(p.sB, p.sB2) + (p.b_kn ? ((int64_t)p.K - 1) * p.ldb + p.N - 1 : ((int64_t)p.N - 1) * p.ldb + p.K - 1);
    o.c = last(p.sC, p.sC2) + ((int64_t)p.M - 1) * p.ldc + p.N - 1;
    o.r = p.residual ? last(p.sR, p.sR2) + ((int64_t)p.M - 1) * p.ldr + p.N - 1 : -1;
    return true;
}

tk_error_code_t tk_mi355x_gemm_probe(int device, tk_mi355x_gemm_probe_t* p) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    p->kernel = TK_GEMM_REFUSED;
    ProbeReach reach;
    if (!p->a || !p->b || !p->c || !probe_reach(*p, reach)) return TK_ERROR_INVALID_ARGUMENT;
    if (p->n_a < 1 || p->n_b < 1 || p->n_c < 1 || reach.a >= p->n_a || reach.b >= p->n_b || reach.c >= p->n_c) return TK_ERROR_INVALID_ARGUMENT;
    if (p->bias ? p->n_bias < p->N : p->n_bias != 0) return TK_ERROR_INVALID_ARGUMENT;
    if (p->residual ? reach.r >= p->n_residual : p->n_residual != 0) return TK_ERROR_INVALID_ARGUMENT;
    const size_t eb = p->b_f16 ? 2 : 4;
    TkGemm g{};
    g.M = p->M; g.N = p->N; g.K = p->K; g.lda = p->lda; g.ldb = p->ldb; g.ldc = p->ldc; g.ldr = p->ldr; g.b_kn = p->b_kn; g.act = p->act; g.alpha = p->alpha;
    g.batch = p->batch; g.sA = p->sA; g.sB = p->sB; g.sC = p->sC; g.sR = p->sR;
    g.batch_inner = p->batch_inner; g.sA2 = p->sA2; g.sB2 = p->sB2; g.sC2 = p->sC2; g.sR2 = p->sR2;
    g.b_f16 = p->b_f16; g.fast = p->fast;
    g.im_C = p->im_C; g.im_H = p->im_H; g.im_W = p->im_W; g.im_ldx = p->im_ldx; g.im_kw = p->im_kw; g.im_stride = p->im_stride; g.im_pad = p->im_pad;
    g.im_Ho = p->im_Ho; g.im_Wo = p->im_Wo;
    if (device < 0) { /* the launcher's answer alone: bases as the device allocator would align them */
        g.A = (const float*)(uintptr_t)256 + p->a_offset;
        g.B = (const float*)((uintptr_t)256 + (size_t)p->b_offset * eb);
        p->kernel = tk_gemm_kernel_of(g);
        return p->kernel < 0 ? TK_ERROR_INVALID_ARGUMENT : TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    if (!tk_nn_prepare_device()) return TK_ERROR_GPU_ROCM_ERROR;
    float *da = nullptr, *dbias = nullptr, *dr = nullptr, *dc = nullptr;
    uint8_t* db = nullptr;
    const size_t ba = ((size_t)p->n_a + p->a_offset) * 4, bb = ((size_t)p->n_b + p->b_offset) * eb;
    bool ok = hipMalloc((void**)&da, ba) == hipSuccess && hipMalloc((void**)&db, bb) == hipSuccess && hipMalloc((void**)&dc, (size_t)p->n_c * 4) == hipSuccess &&
              (!p->bias || hipMalloc((void**)&dbias, (size_t)p->n_bias * 4) == hipSuccess) &&
              (!p->residual || hipMalloc((void**)&dr, (size_t)p->n_residual * 4) == hipSuccess);
    ok = ok && hipMemcpy(da + p->a_offset, p->a, (size_t)p->n_a * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(db + (size_t)p->b_offset * eb, p->b, (size_t)p->n_b * eb, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dc, p->c, (size_t)p->n_c * 4, hipMemcpyHostToDevice) == hipSuccess &&
         (!p->bias || hipMemcpy(dbias, p->bias, (size_t)p->n_bias * 4, hipMemcpyHostToDevice) == hipSuccess) &&
         (!p->residual || hipMemcpy(dr, p->residual, (size_t)p->n_residual * 4, hipMemcpyHostToDevice) == hipSuccess);
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        g.A = da + p->a_offset; g.B = (const float*)(db + (size_t)p->b_offset * eb); g.C = dc; g.bias = dbias; g.residual = dr;
        p->kernel = tk_gemm_kernel_of(g);
        if (!tk_launch_gemm(g, nullptr)) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(p->c, dc, (size_t)p->n_c * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    void* ptrs[] = {da, db, dbias, dr, dc};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    return rc;
}

tk_error_code_t tk_mi355x_attention_h3_probe(int device, int B, int nh, int Tq, int Tk, int64_t q_bstride, int64_t kv_bstride, int d, float scale, const float* q,
                                             const float* k, const float* v, int64_t n_q, int64_t n_kv, float* out) {
    const int64_t cap = (int64_t)1 << 28;
    if (!q || !k || !v || !out || B < 1 || B > 4096 || nh < 1 || nh > 4096 || Tq < 1 || Tq > cap || Tk < 1 || Tk > cap || d < 1 || d > cap || q_bstride < 0 ||
        q_bstride > cap || kv_bstride < 0 || kv_bstride > cap)
        return TK_ERROR_INVALID_ARGUMENT;
    /* what the launcher refuses, before any device work (it checks the same and the bases' alignment) */
    if (d != nh * 64 || (q_bstride & 3) || (kv_bstride & 3)) return TK_ERROR_INVALID_ARGUMENT;
    if ((B - 1) * q_bstride + (int64_t)Tq * d > n_q || (B - 1) * kv_bstride + (int64_t)Tk * d > n_kv) return TK_ERROR_INVALID_ARGUMENT;
    if (B > 1 && (q_bstride < (int64_t)Tq * d || kv_bstride < (int64_t)Tk * d)) return TK_ERROR_INVALID_ARGUMENT; /* sequences would overlap */
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    float *dq = nullptr, *dk = nullptr, *dv = nullptr, *dout = nullptr;
    bool ok = hipMalloc((void**)&dq, (size_t)n_q * 4) == hipSuccess && hipMalloc((void**)&dk, (size_t)n_kv * 4) == hipSuccess &&
              hipMalloc((void**)&dv, (size_t)n_kv * 4) == hipSuccess && hipMalloc((void**)&dout, (size_t)n_q * 4) == hipSuccess;
    ok = ok && hipMemcpy(dq, q, (size_t)n_q * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dk, k, (size_t)n_kv * 4, hipMemcpyHostToDevice) == hipSuccess &&
         hipMemcpy(dv, v, (size_t)n_kv * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(dout, out, (size_t)n_q * 4, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        if (!tk_launch_attention_h3(dq, dk, dv, dout, B, nh, Tq, Tk, q_bstride, kv_bstride, d, scale, nullptr)) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(out, dout, (size_t)n_q * 4, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    void* ptrs[] = {dq, dk, dv, dout};
    for (void* p : ptrs) if (p) (void)hipFree(p);
    return rc;
}

/* what a token-pick launch may be handed (tk_mi355x_ext.h states the rules); false: refuse */
static bool pick_probe_ok(const tk_mi355x_token_pick_probe_t& p) {
    static_assert(sizeof(tk_mi355x_sampling_t) == sizeof(TkSampleRow), "the public sampling state is the kernels' TkSampleRow");
    const bool llm = p.kind == TK_MI355X_PICK_ARGMAX;
    if (p.kind < TK_MI355X_PICK_ARGMAX || p.kind > TK_MI355X_PICK_ROWS_FILTERED || !p.logits) return false;
    if (p.rows < 1 || p.rows > (llm ? TK_MAX_ROWS : 4096) || p.cols < 1 || p.cols > (1 << 24) || p.ld < p.cols || p.ld > (1 << 24) || (llm && p.ld != p.cols)) return false;
    if (p.n_logits < (int64_t)(p.rows - 1) * p.ld + p.cols) return false;
    const bool wide = p.cols > 65536;
    if (llm) {
        if (p.n_masks < 0 || (p.masks == nullptr) != (p.n_masks == 0)) return false;
        if (p.allow_row)
            for (int r = 0; r < p.rows; ++r)
                if (p.allow_row[r] < -1 || p.allow_row[r] >= p.n_masks) return false;
        if (p.samp)
            for (int r = 0; r < p.rows; ++r) {
                const float t = p.samp[r].temperature;
                if (!isfinite(t) || t < 0.0f || (t > 0.0f && wide)) return false;
            }
        if (p.hist) {
            if (!p.nsteps || p.hist_stride < p.rows || p.n_hist < 1) return false;
            for (int r = 0; r < p.rows; ++r)
                if (p.nsteps[r] < 0 || (int64_t)p.nsteps[r] * p.hist_stride + r >= p.n_hist) return false;
        }
        return true;
    }
    if (!p.tok || !isfinite(p.temperature) || p.temperature < 0.0f) return false;
    if (p.kind == TK_MI355X_PICK_ARGMAX_ROWS) return p.logprob == nullptr;
    if (p.kind == TK_MI355X_PICK_ROWS) return !(wide && p.temperature > 0.0f);
    if (wide || !p.suppress || !p.state || p.beg < 0 || p.beg > p.cols || p.eot < 0 || p.eot >= p.cols || p.tid0 < -1 || p.tid0 > p.cols) return false;
    for (int r = 0; r < p.rows; ++r) {
        const int32_t* st = p.state + (int64_t)r * TK_WH_STATE_INTS;
        const int32_t counts[4] = {st[0], st[4], st[5], st[7]};
        for (int32_t v : counts) if (v < 0 || v > (1 << 24)) return false;
        if (st[6] != 0) continue; /* stands still: reads no logit */
        /* the kernel's allowed set A0: empty, its pick stays 0x7fffffff and logits[pick] is read; so it does when every allowed logit is a NaN */
        const int n_tok = st[0], last_ts = n_tok > 0 ? st[1] : 0, prev_ts = n_tok < 2 ? 1 : st[2];
        const int ts_lo = st[3] ? p.beg + st[4] / 2 : p.beg, ts_hi = n_tok == 0 && p.tid0 >= 0 ? p.beg + p.tid0 : 0x7fffffff;
        bool any = false;
        for (int i = 0; i < p.cols; ++i) {
            const float v = p.logits[(int64_t)r * p.ld + i];
            if (v != v) return false;
            bool ok = p.suppress[i] == 0;
            if (i >= p.beg) ok = ok && i >= ts_lo && i <= ts_hi && !(last_ts && prev_ts);
            if (last_ts && !prev_ts && i < p.eot) ok = false;
            any = any || ok;
        }
        if (!any) return false;
    }
    return true;
}

tk_error_code_t tk_mi355x_token_pick_probe(int device, tk_mi355x_token_pick_probe_t* p) {
    if (!p || !pick_probe_ok(*p)) return TK_ERROR_INVALID_ARGUMENT;
    if (device < 0) return TK_SUCCESS;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    const size_t rows = (size_t)p->rows, mask_words = (size_t)p->n_masks * (size_t)((p->cols + 31) / 32);
    /* host array, bytes, device copy, read back after the launch */
    struct Buf { const void* host; size_t bytes; void* dev; bool out; };
    Buf b[] = {{p->logits, (size_t)p->n_logits * 4, nullptr, false}, {p->masks, mask_words * 4, nullptr, false}, {p->allow_row, rows * 4, nullptr, false},
               {p->samp, rows * sizeof(TkSampleRow), nullptr, true}, {p->tok, rows * 4, nullptr, true}, {p->pos, rows * 4, nullptr, true},
               {p->nsteps, rows * 4, nullptr, true}, {p->hist, (size_t)p->n_hist * 4, nullptr, true}, {p->logprob, rows * 4, nullptr, true},
               {p->suppress, (size_t)p->cols, nullptr, false}, {p->state, rows * TK_WH_STATE_INTS * 4, nullptr, true}};
    enum { LOGITS, MASKS, ALLOW_ROW, SAMP, TOK, POS, NSTEPS, HIST, LOGPROB, SUPPRESS, STATE };
    const bool llm = p->kind == TK_MI355X_PICK_ARGMAX;
    bool ok = true;
    for (Buf& q : b) {
        const int which = (int)(&q - b);
        const bool used = q.host && (llm ? which <= HIST : which == LOGITS || which == TOK || which == LOGPROB || (p->kind == TK_MI355X_PICK_ROWS_FILTERED && which >= SUPPRESS));
        if (!used) { q.host = nullptr; continue; }
        ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess;
    }
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        const float* x = (const float*)b[LOGITS].dev;
        const TkPick pk{p->temperature, p->seed, p->counter0, (float*)b[LOGPROB].dev};
        if (llm)
            tk_launch_argmax(x, p->cols, p->rows, (const uint32_t*)b[MASKS].dev, (const int32_t*)b[ALLOW_ROW].dev, (TkSampleRow*)b[SAMP].dev, (int32_t*)b[TOK].dev,
                             (int32_t*)b[POS].dev, (int32_t*)b[NSTEPS].dev, (int32_t*)b[HIST].dev, p->hist_stride, nullptr);
        else if (p->kind == TK_MI355X_PICK_ARGMAX_ROWS) tk_launch_argmax_rows(x, p->rows, p->cols, p->ld, (int32_t*)b[TOK].dev, nullptr);
        else if (p->kind == TK_MI355X_PICK_ROWS) tk_launch_pick_rows(x, p->rows, p->cols, p->ld, (int32_t*)b[TOK].dev, pk, nullptr);
        else {
            const TkWhFilter f{(const uint8_t*)b[SUPPRESS].dev, (int32_t*)b[STATE].dev, p->beg, p->eot, p->tid0};
            tk_launch_pick_rows_filtered(x, p->rows, p->cols, p->ld, (int32_t*)b[TOK].dev, pk, f, nullptr);
        }
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        else
            for (Buf& q : b)
                if (q.host && q.out && hipMemcpy(const_cast<void*>(q.host), q.dev, q.bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

static_assert(sizeof(tk_mi355x_logit_adjust_t) == sizeof(TkLogitAdjust) && offsetof(tk_mi355x_logit_adjust_t, recent) == offsetof(TkLogitAdjust, recent) &&
                  offsetof(tk_mi355x_logit_adjust_t, n_bias) == offsetof(TkLogitAdjust, n_bias) && offsetof(tk_mi355x_logit_adjust_t, bias) == offsetof(TkLogitAdjust, bias),
              "the public logit adjustment is the library's TkLogitAdjust");

tk_error_code_t tk_mi355x_logit_adjust_probe(int device, int32_t rows, int32_t cols, float* logits, int64_t n_logits, const tk_mi355x_logit_adjust_t* adjust) {
    if (!logits || !adjust || rows < 1 || rows > TK_MAX_ROWS || cols < 1 || cols > (1 << 24) || n_logits < (int64_t)rows * cols) return TK_ERROR_INVALID_ARGUMENT;
    const TkLogitAdjust* adj = (const TkLogitAdjust*)adjust;
    for (int r = 0; r < rows; ++r)
        if (adj[r].check(cols)) return TK_ERROR_INVALID_ARGUMENT;
    if (device < 0) {
        for (int r = 0; r < rows; ++r) tk_logit_adjust_row(logits + (int64_t)r * cols, adj[r].row(), adj[r].recent, adj[r].bias_ids, adj[r].bias);
        return TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    /* the session's tables (TkLlmSession::forward): descriptors, then windows, bias ids and bias values of TK_ADJUST_MAX_* entries per row */
    std::vector<TkAdjustRow> desc((size_t)rows);
    std::vector<int32_t> ids((size_t)rows * TK_ADJUST_MAX_RECENT, 0), bids((size_t)rows * TK_ADJUST_MAX_BIAS, 0);
    std::vector<float> bias((size_t)rows * TK_ADJUST_MAX_BIAS, 0.0f);
    for (int r = 0; r < rows; ++r) {
        desc[(size_t)r] = adj[r].row();
        for (int j = 0; j < adj[r].n_recent; ++j) ids[(size_t)r * TK_ADJUST_MAX_RECENT + j] = adj[r].recent[j];
        for (int j = 0; j < adj[r].n_bias; ++j) { bids[(size_t)r * TK_ADJUST_MAX_BIAS + j] = adj[r].bias_ids[j]; bias[(size_t)r * TK_ADJUST_MAX_BIAS + j] = adj[r].bias[j]; }
    }
    struct Buf { const void* host; size_t bytes; void* dev; };
    Buf b[] = {{logits, (size_t)n_logits * 4, nullptr}, {desc.data(), desc.size() * sizeof(TkAdjustRow), nullptr}, {ids.data(), ids.size() * 4, nullptr},
               {bids.data(), bids.size() * 4, nullptr}, {bias.data(), bias.size() * 4, nullptr}};
    bool ok = true;
    for (Buf& q : b) ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        tk_launch_logit_adjust((float*)b[0].dev, cols, rows, (const TkAdjustRow*)b[1].dev, (const int32_t*)b[2].dev, (const int32_t*)b[3].dev, (const float*)b[4].dev, nullptr);
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(logits, b[0].dev, b[0].bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

static_assert(sizeof(tk_mi355x_token_logprob_t) == sizeof(TkTokenLogprob) && offsetof(tk_mi355x_token_logprob_t, n_top) == offsetof(TkTokenLogprob, n_top) &&
                  offsetof(tk_mi355x_token_logprob_t, top_ids) == offsetof(TkTokenLogprob, top_ids) &&
                  offsetof(tk_mi355x_token_logprob_t, top_logprobs) == offsetof(TkTokenLogprob, top_logprobs) && TK_MI355X_LOGPROB_MAX_TOP == TK_LOGPROB_MAX_TOP,
              "the public log-probability record is the library's TkTokenLogprob");

tk_error_code_t tk_mi355x_token_logprobs_probe(int device, int32_t rows, int32_t cols, int32_t ld, const float* logits, int64_t n_logits, const int32_t* ids,
                                               const int32_t* n_top, tk_mi355x_token_logprob_t* records) {
    if (!logits || !ids || !n_top || !records || rows < 1 || rows > TK_MAX_ROWS || cols < 1 || cols > TK_LOGPROB_MAX_VOCAB || ld < cols || ld > (1 << 24) ||
        n_logits < (int64_t)(rows - 1) * ld + cols)
        return TK_ERROR_INVALID_ARGUMENT;
    for (int r = 0; r < rows; ++r) {
        if (tk_logprob_check(n_top[r], cols) || ids[r] < 0 || ids[r] >= cols) return TK_ERROR_INVALID_ARGUMENT;
        if (n_top[r] >= 0 && tk_logprob_check_row(logits + (int64_t)r * ld, cols)) return TK_ERROR_INVALID_ARGUMENT;
    }
    TkTokenLogprob* rec = (TkTokenLogprob*)records;
    if (device < 0) {
        for (int r = 0; r < rows; ++r) tk_token_logprob_row(logits + (int64_t)r * ld, cols, ids[r], n_top[r], rec + r);
        return TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    struct Buf { const void* host; size_t bytes; void* dev; };
    Buf b[] = {{logits, (size_t)n_logits * 4, nullptr}, {ids, (size_t)rows * 4, nullptr}, {n_top, (size_t)rows * 4, nullptr}, {rec, (size_t)rows * sizeof(TkTokenLogprob), nullptr}};
    bool ok = true;
    for (Buf& q : b) ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        tk_launch_token_logprobs((const float*)b[0].dev, cols, ld, rows, (const int32_t*)b[2].dev, (const int32_t*)b[1].dev, (TkTokenLogprob*)b[3].dev, nullptr);
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || hipMemcpy(rec, b[3].dev, b[3].bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

/* stand-alone timing of that launch (tools/time_token_logprobs.py): rows x cols logits from a fixed generator, every row with the same n_top and chosen
 * id 0; `iters` launches after one untimed launch, device events around them; average ms of one */
tk_error_code_t tk_mi355x_time_token_logprobs(int device, int32_t rows, int32_t cols, int32_t n_top, int32_t iters, float* avg_ms) {
    if (!avg_ms || rows < 1 || rows > TK_MAX_ROWS || cols < 1 || cols > TK_LOGPROB_MAX_VOCAB || n_top < 0 || n_top > TK_LOGPROB_MAX_TOP || iters < 1 || iters > 100000)
        return TK_ERROR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device < 0 || device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    std::vector<float> lg((size_t)rows * cols);
    uint64_t z = 0x9E3779B97F4A7C15ull;
    for (float& v : lg) { /* logits spread over [-8, 8) */
        z = z * 6364136223846793005ull + 1442695040888963407ull;
        v = (float)(uint32_t)(z >> 40) * (16.0f / 16777216.0f) - 8.0f;
    }
    std::vector<int32_t> ids((size_t)rows, 0), nt((size_t)rows, n_top);
    void *d_lg = nullptr, *d_ids = nullptr, *d_nt = nullptr, *d_rec = nullptr;
    hipEvent_t e0 = nullptr, e1 = nullptr;
    bool ok = hipMalloc(&d_lg, lg.size() * 4) == hipSuccess && hipMalloc(&d_ids, ids.size() * 4) == hipSuccess && hipMalloc(&d_nt, nt.size() * 4) == hipSuccess &&
              hipMalloc(&d_rec, (size_t)rows * sizeof(TkTokenLogprob)) == hipSuccess && hipMemcpy(d_lg, lg.data(), lg.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipMemcpy(d_ids, ids.data(), ids.size() * 4, hipMemcpyHostToDevice) == hipSuccess && hipMemcpy(d_nt, nt.data(), nt.size() * 4, hipMemcpyHostToDevice) == hipSuccess &&
              hipEventCreate(&e0) == hipSuccess && hipEventCreate(&e1) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        tk_launch_token_logprobs((const float*)d_lg, cols, cols, rows, (const int32_t*)d_nt, (const int32_t*)d_ids, (TkTokenLogprob*)d_rec, nullptr);
        (void)hipEventRecord(e0, nullptr);
        for (int i = 0; i < iters; ++i) tk_launch_token_logprobs((const float*)d_lg, cols, cols, rows, (const int32_t*)d_nt, (const int32_t*)d_ids, (TkTokenLogprob*)d_rec, nullptr);
        (void)hipEventRecord(e1, nullptr);
        float ms = 0.0f;
        if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipEventSynchronize(e1) != hipSuccess || hipEventElapsedTime(&ms, e0, e1) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        else *avg_ms = ms / (float)iters;
    }
    if (e0) (void)hipEventDestroy(e0);
    if (e1) (void)hipEventDestroy(e1);
    void* ptrs[] = {d_lg, d_ids, d_nt, d_rec};
    for (void* q : ptrs) if (q) (void)hipFree(q);
    return rc;
}

tk_error_code_t tk_mi355x_kv_shift_probe(int device, int32_t n_layer, int32_t max_seq, int32_t n_kv_head, int32_t max_ctx, int32_t head_dim, uint16_t* kcache,
                                         uint16_t* vcache, const float* rope_cos, const float* rope_sin, int32_t seq, int32_t p0, int32_t p1, int32_t delta) {
    const int32_t cap = 1 << 16;
    if (!kcache || !vcache || !rope_cos || !rope_sin || n_layer < 1 || n_layer > cap || max_seq < 1 || max_seq > cap || n_kv_head < 1 || n_kv_head > cap || max_ctx < 1 ||
        max_ctx > cap || head_dim < 8 || head_dim > 256 || head_dim % 8 != 0)
        return TK_ERROR_INVALID_ARGUMENT;
    const TkKvShiftDesc m{seq, p0, p1, delta};
    if (!tk_kv_shift_ok(m, max_seq, max_ctx)) return TK_ERROR_INVALID_ARGUMENT;
    const int64_t elems = (int64_t)n_layer * max_seq * n_kv_head * max_ctx * head_dim;
    if (elems > ((int64_t)1 << 31)) return TK_ERROR_INVALID_ARGUMENT;
    if (device < 0) {
        for (int layer = 0; layer < n_layer; ++layer)
            for (int kvh = 0; kvh < n_kv_head; ++kvh) {
                const size_t run = (((size_t)layer * max_seq + seq) * n_kv_head + kvh) * max_ctx * head_dim;
                tk_kv_shift_run(kcache + run, true, m, head_dim, rope_cos, rope_sin);
                tk_kv_shift_run(vcache + run, false, m, head_dim, rope_cos, rope_sin);
            }
        return TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    const size_t table = (size_t)max_ctx * (head_dim / 2) * 4;
    struct Buf { const void* host; size_t bytes; void* dev; bool out; };
    Buf b[] = {{kcache, (size_t)elems * 2, nullptr, true}, {vcache, (size_t)elems * 2, nullptr, true}, {rope_cos, table, nullptr, false}, {rope_sin, table, nullptr, false}};
    bool ok = true;
    for (Buf& q : b) ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        if (!tk_launch_kv_shift_rows(m, (uint16_t*)b[0].dev, (uint16_t*)b[1].dev, (const float*)b[2].dev, (const float*)b[3].dev, n_layer, n_kv_head, head_dim, max_seq,
                                     max_ctx, nullptr)) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        else
            for (Buf& q : b)
                if (q.out && hipMemcpy(const_cast<void*>(q.host), q.dev, q.bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

tk_error_code_t tk_mi355x_lang_pick_probe(int device, int32_t rows, int32_t cols, int32_t ld, const float* logits, int64_t n_logits, int32_t tok0, int32_t n_lang,
                                          const int32_t* auto_row, int32_t* slot, int32_t* ids, float* probs) {
    if (!logits || !auto_row || !slot || !ids || !probs || tk_lang_pick_check(rows, cols, ld, tok0, n_lang)) return TK_ERROR_INVALID_ARGUMENT;
    if (n_logits < (int64_t)(rows - 1) * ld + cols) return TK_ERROR_INVALID_ARGUMENT;
    for (int r = 0; r < rows; ++r)
        for (int i = 0; i < n_lang; ++i)
            if (logits[(int64_t)r * ld + tok0 + i] > 3.402823466e38f) return TK_ERROR_INVALID_ARGUMENT; /* +inf: inf - inf has no probability */
    if (device < 0) {
        for (int r = 0; r < rows; ++r) {
            ids[r] = tk_lang_pick_row(logits + (int64_t)r * ld + tok0, n_lang, nullptr, probs + (int64_t)r * n_lang);
            if (auto_row[r] != 0) slot[r] = tok0 + ids[r];
        }
        return TK_SUCCESS;
    }
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    std::vector<float> pid((size_t)rows);
    /* host array, bytes, device copy, read back after the launch */
    struct Buf { const void* host; size_t bytes; void* dev; bool out; };
    Buf b[] = {{logits, (size_t)n_logits * 4, nullptr, false}, {auto_row, (size_t)rows * 4, nullptr, false}, {slot, (size_t)rows * 4, nullptr, true},
               {ids, (size_t)rows * 4, nullptr, true}, {pid.data(), (size_t)rows * 4, nullptr, true}, {probs, (size_t)rows * n_lang * 4, nullptr, true}};
    bool ok = true;
    for (Buf& q : b) ok = ok && hipMalloc(&q.dev, q.bytes) == hipSuccess && hipMemcpy(q.dev, q.host, q.bytes, hipMemcpyHostToDevice) == hipSuccess;
    tk_error_code_t rc = ok ? TK_SUCCESS : TK_ERROR_GPU_ROCM_ERROR;
    if (ok) {
        if (!tk_launch_lang_pick((const float*)b[0].dev, rows, cols, ld, tok0, n_lang, (const int32_t*)b[1].dev, (int32_t*)b[2].dev, (int32_t*)b[3].dev, (float*)b[4].dev,
                                 (float*)b[5].dev, nullptr)) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        else
            for (Buf& q : b)
                if (q.out && hipMemcpy(const_cast<void*>(q.host), q.dev, q.bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = TK_ERROR_GPU_ROCM_ERROR;
        /* the kernel's own prob[id] is the engine's per-row answer: it must be the row's entry of probs */
        for (int r = 0; rc == TK_SUCCESS && r < rows; ++r)
            if (tk_f32_bits(pid[(size_t)r]) != tk_f32_bits(probs[(int64_t)r * n_lang + ids[r]])) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    for (Buf& q : b) if (q.dev) (void)hipFree(q.dev);
    return rc;
}

/* one host array of a probe: where it comes from, how many bytes, how far into its device allocation it is placed, whether it is read back */
struct ProbeBuf { const void* host; size_t bytes, offset; bool out; void* dev; };
static bool probe_upload(ProbeBuf* b, int n) {
    for (int i = 0; i < n; ++i) {
        if (!b[i].host) continue;
        if (hipMalloc(&b[i].dev, b[i].bytes + b[i].offset) != hipSuccess) return false;
        if (hipMemcpy((uint8_t*)b[i].dev + b[i].offset, b[i].host, b[i].bytes, hipMemcpyHostToDevice) != hipSuccess) return false;
    }
    return true;
}
static bool probe_download(ProbeBuf* b, int n) {
    bool ok = true;
    for (int i = 0; i < n; ++i)
        if (b[i].host && b[i].out && hipMemcpy(const_cast<void*>(b[i].host), (uint8_t*)b[i].dev + b[i].offset, b[i].bytes, hipMemcpyDeviceToHost) != hipSuccess) ok = false;
    return ok;
}
static void probe_free(ProbeBuf* b, int n) {
    for (int i = 0; i < n; ++i) if (b[i].dev) (void)hipFree(b[i].dev);
}
static tk_error_code_t probe_device(int device) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (device >= n || hipSetDevice(device) != hipSuccess) return TK_ERROR_INVALID_ARGUMENT;
    return TK_SUCCESS;
}

/* floats each array of a row-probe launch must hold (0: not read), from the kernels' own index expressions; false: a geometry no launch may have */
struct RowReach { int64_t a, b, c, idx, y, img; };
static bool row_probe_reach(const tk_mi355x_nn_row_probe_t& p, RowReach& o) {
    const int64_t cap = (int64_t)1 << 20, big = (int64_t)1 << 28;
    auto dim = [&](int64_t v) { return v >= 1 && v <= cap; };
    o = RowReach{0, 0, 0, 0, 0, 0};
    if (p.a_offset < 0 || p.a_offset > 64 || p.y_offset < 0 || p.y_offset > 64) return false;
    if (p.op == TK_MI355X_ROW_ATTEND1) {
        if (!dim(p.B) || !dim(p.H) || !dim(p.C) || !dim(p.N) || p.q_bstride < 0 || p.q_bstride > big || p.kv_bstride < 0 || p.kv_bstride > big) return false;
        if (p.B > 1 && p.q_bstride < p.C) return false; /* output rows would overlap */
        const int64_t q_need = ((int64_t)p.B - 1) * p.q_bstride + p.C, kv_need = ((int64_t)p.B - 1) * p.kv_bstride + (int64_t)p.H * p.C;
        if (q_need > big || kv_need > big) return false;
        o.a = q_need; o.b = kv_need; o.c = kv_need; o.y = q_need;
        if (p.img) o.img = (((int64_t)p.B + 15) / 16) * 16 * p.C;
        return true;
    }
    const bool image = p.op <= TK_MI355X_ROW_UPSAMPLE2X;
    if (image) {
        const int W = p.op == TK_MI355X_ROW_IM2COL1D ? 1 : p.W;
        if (!dim(p.B) || !dim(p.H) || !dim(W) || !dim(p.C) || !dim(p.ldx) || p.ldx < p.C) return false;
        const int64_t pixels = (int64_t)p.B * p.H * W;
        if (pixels > big || pixels * p.ldx > big) return false;
        o.a = (pixels - 1) * p.ldx + p.C;
        if (p.op <= TK_MI355X_ROW_IM2COL1D) {
            if (!dim(p.k) || !dim(p.stride) || p.pad < 0 || p.pad > cap || p.H + 2 * (int64_t)p.pad < p.k || (p.op != TK_MI355X_ROW_IM2COL1D && W + 2 * (int64_t)p.pad < p.k)) return false;
            const int64_t Ho = (p.H + 2 * (int64_t)p.pad - p.k) / p.stride + 1, Wo = p.op == TK_MI355X_ROW_IM2COL1D ? 1 : (W + 2 * (int64_t)p.pad - p.k) / p.stride + 1;
            const int64_t K = (int64_t)p.k * (p.op == TK_MI355X_ROW_IM2COL1D ? 1 : p.k) * p.C, opix = (int64_t)p.B * Ho * Wo;
            if (opix > big || K > big || opix * K > big) return false;
            if (p.op == TK_MI355X_ROW_CONV_STEM) {
                if (!dim(p.N) || !dim(p.ldy) || p.ldy < p.N || (p.act != TK_ACT_NONE && p.act != TK_ACT_SILU) || opix * p.ldy > big || K * p.N > big) return false;
                o.b = K * p.N;
                o.c = p.N;
                o.y = (opix - 1) * p.ldy + p.N;
            } else o.y = opix * K;
        } else {
            if (!dim(p.ldy) || p.ldy < p.C) return false;
            const int64_t opix = p.op == TK_MI355X_ROW_UPSAMPLE2X ? 4 * pixels : pixels;
            if (opix * p.ldy > big) return false;
            o.y = (opix - 1) * p.ldy + p.C;
        }
        return true;
    }
    if (!dim(p.rows) || !dim(p.C)) return false;
    const int64_t packed = (int64_t)p.rows * p.C;
    if (packed > big) return false;
    switch (p.op) {
    case TK_MI355X_ROW_COPY_COLS:
        if (!dim(p.ldx) || !dim(p.ldy) || p.ldx < p.C || p.ldy < p.C || (int64_t)p.rows * p.ldx > big || (int64_t)p.rows * p.ldy > big) return false;
        o.a = ((int64_t)p.rows - 1) * p.ldx + p.C;
        o.y = ((int64_t)p.rows - 1) * p.ldy + p.C;
        return true;
    case TK_MI355X_ROW_LAYERNORM:
        if (!(p.eps >= 0.0f) || !(p.eps < 1.0f)) return false;
        o.a = packed; o.b = p.C; o.c = p.C; o.y = packed;
        if (p.img) {
            if (p.C & 15) return false; /* the launcher refuses it too: 16-row blocks of the image would overlap */
            o.img = (((int64_t)p.rows + 15) / 16) * 16 * p.C;
        }
        return true;
    case TK_MI355X_ROW_SOFTMAX_ROWS:
        if (!dim(p.ldy) || p.ldy < p.C || (int64_t)p.rows * p.ldy > big) return false;
        o.y = ((int64_t)p.rows - 1) * p.ldy + p.C;
        return true;
    case TK_MI355X_ROW_ADD_ROWS:
        if (!dim(p.add_rows) || (int64_t)p.add_rows * p.C > big) return false;
        o.a = (int64_t)p.add_rows * p.C; o.y = packed;
        return true;
    case TK_MI355X_ROW_EMBED_ROWS:
        if (!dim(p.table_rows) || !dim(p.pos_rows) || (int64_t)p.table_rows * p.C > big || (int64_t)p.pos_rows * p.C > big) return false;
        o.a = (int64_t)p.table_rows * p.C; o.b = (int64_t)p.pos_rows * p.C; o.idx = p.rows; o.y = packed;
        return true;
    default: return false;
    }
}

/* the launch itself (or, with s_dry, the launcher's kernel code alone) on the given bases; false: the launcher refuses */
static bool row_probe_launch(tk_mi355x_nn_row_probe_t& p, const float* a, const float* b, const float* c, const int32_t* idx, const int32_t* pos_idx, float* y, float* img,
                             bool dry) {
    p.kernel = 0;
    switch (p.op) {
    case TK_MI355X_ROW_CONV_STEM:
        if (!tk_conv_stem_ok(p.B, p.H, p.W, p.C, p.ldx, p.N, p.k, p.stride, p.pad, y, p.ldy)) { p.kernel = -1; return false; }
        if (dry) return true;
        if (!tk_launch_conv_stem(a, p.B, p.H, p.W, p.C, p.ldx, b, c, p.act, p.N, p.k, p.stride, p.pad, y, p.ldy, nullptr)) { p.kernel = -1; return false; }
        return true;
    case TK_MI355X_ROW_IM2COL:
        p.kernel = tk_im2col_kernel_of(a, p.B, p.H, p.W, p.C, p.ldx, p.k, p.k, p.stride, p.pad, y);
        return p.kernel >= 0 && (dry || tk_launch_im2col(a, p.B, p.H, p.W, p.C, p.ldx, p.k, p.k, p.stride, p.pad, y, nullptr));
    case TK_MI355X_ROW_IM2COL1D: return dry || tk_launch_im2col1d(a, p.B, p.H, p.C, p.ldx, p.k, p.stride, p.pad, y, nullptr);
    case TK_MI355X_ROW_MAXPOOL5: return dry || tk_launch_maxpool5(a, p.B, p.H, p.W, p.C, p.ldx, y, p.ldy, nullptr);
    case TK_MI355X_ROW_UPSAMPLE2X: return dry || tk_launch_upsample2x(a, p.B, p.H, p.W, p.C, p.ldx, y, p.ldy, nullptr);
    case TK_MI355X_ROW_COPY_COLS: return dry || tk_launch_copy_cols(a, p.rows, p.C, p.ldx, y, p.ldy, nullptr);
    case TK_MI355X_ROW_LAYERNORM: return dry || tk_launch_layernorm(a, p.rows, p.C, b, c, p.eps, y, nullptr, img);
    case TK_MI355X_ROW_SOFTMAX_ROWS:
        p.kernel = tk_softmax_kernel_of(p.rows, p.C, p.ldy, y);
        return p.kernel >= 0 && (dry || tk_launch_softmax_rows(y, p.rows, p.C, p.ldy, nullptr));
    case TK_MI355X_ROW_ADD_ROWS: return dry || tk_launch_add_rows(y, a, p.rows, p.C, p.add_rows, nullptr);
    case TK_MI355X_ROW_EMBED_ROWS: return dry || tk_launch_embed_rows(a, b, idx, pos_idx, p.rows, p.C, y, nullptr);
    case TK_MI355X_ROW_ATTEND1:
        if (!tk_attend1_ok(b, c, p.B, p.H, p.q_bstride, p.kv_bstride, p.C, p.N)) { p.kernel = -1; return false; }
        return dry || tk_launch_attend1(a, b, c, y, p.B, p.H, p.q_bstride, p.kv_bstride, p.C, p.N, img, nullptr);
    default: return false;
    }
}

tk_error_code_t tk_mi355x_nn_row_probe(int device, tk_mi355x_nn_row_probe_t* p) {
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    p->kernel = -1;
    RowReach need;
    if (p->op < TK_MI355X_ROW_CONV_STEM || p->op > TK_MI355X_ROW_ATTEND1 || !row_probe_reach(*p, need)) return TK_ERROR_INVALID_ARGUMENT;
    /* an array the op reads must be there and long enough; one it does not read must be absent (bias of the stem: the caller's choice) */
    auto fits = [](const void* ptr, int64_t n, int64_t want, bool optional) {
        if (want == 0) return ptr == nullptr && n == 0;
        if (!ptr) return optional && n == 0;
        return n >= want;
    };
    if (!fits(p->a, p->n_a, need.a, false) || !fits(p->b, p->n_b, need.b, false) || !fits(p->c, p->n_c, need.c, p->op == TK_MI355X_ROW_CONV_STEM) ||
        !fits(p->idx, p->n_idx, need.idx, false) || !fits(p->pos_idx, p->pos_idx ? p->n_idx : 0, need.idx, false) || !fits(p->y, p->n_y, need.y, false) ||
        !fits(p->img, p->n_img, need.img, true))
        return TK_ERROR_INVALID_ARGUMENT;
    if (p->op == TK_MI355X_ROW_EMBED_ROWS)
        for (int r = 0; r < p->rows; ++r)
            if (p->idx[r] < 0 || p->idx[r] >= p->table_rows || p->pos_idx[r] < 0 || p->pos_idx[r] >= p->pos_rows) return TK_ERROR_INVALID_ARGUMENT;
    if (device < 0) { /* bases as the device allocator aligns them */
        const float* a = p->a ? (const float*)(uintptr_t)256 + p->a_offset : nullptr;
        const float* aligned = (const float*)(uintptr_t)256;
        return row_probe_launch(*p, a, aligned, aligned, nullptr, nullptr, (float*)(uintptr_t)256 + p->y_offset, nullptr, true) ? TK_SUCCESS : TK_ERROR_INVALID_ARGUMENT;
    }
    tk_error_code_t rc = probe_device(device);
    if (rc != TK_SUCCESS) return rc;
    enum { A, Bm, Cm, IDX, POS, Y, IMG, NBUF };
    ProbeBuf b[NBUF] = {{p->a, (size_t)p->n_a * 4, (size_t)p->a_offset * 4, false, nullptr}, {p->b, (size_t)p->n_b * 4, 0, false, nullptr},
                        {p->c, (size_t)p->n_c * 4, 0, false, nullptr}, {p->idx, (size_t)p->n_idx * 4, 0, false, nullptr},
                        {p->pos_idx, (size_t)p->n_idx * 4, 0, false, nullptr}, {p->y, (size_t)p->n_y * 4, (size_t)p->y_offset * 4, true, nullptr},
                        {p->img, (size_t)p->n_img * 4, 0, true, nullptr}};
    if (!probe_upload(b, NBUF)) rc = TK_ERROR_GPU_ROCM_ERROR;
    else {
        auto at = [&](int i) { return b[i].dev ? (float*)((uint8_t*)b[i].dev + b[i].offset) : nullptr; };
        if (!row_probe_launch(*p, at(A), at(Bm), at(Cm), (const int32_t*)b[IDX].dev, (const int32_t*)b[POS].dev, at(Y), at(IMG), false)) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || !probe_download(b, NBUF)) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    probe_free(b, NBUF);
    return rc;
}

/* elements each array of an edge-probe launch must hold (0: not used) and the bytes of one element, from the kernels' own index expressions;
 * false: a geometry no launch may have */
struct EdgeReach { int64_t a, b, c, y, y2; int sa, sb, sy; };
static bool edge_probe_reach(const tk_mi355x_edge_probe_t& p, EdgeReach& o) {
    const int64_t cap = (int64_t)1 << 20, big = (int64_t)1 << 28;
    auto dim = [&](int64_t v) { return v >= 1 && v <= cap; };
    auto finite = [](float v) { return v - v == 0.0f; };
    o = EdgeReach{0, 0, 0, 0, 0, 4, 4, 4};
    switch (p.op) {
    case TK_MI355X_EDGE_FRAMES: {
        /* taps run from -NFFT/2 to (T - 1) HOP + NFFT/2 - 1: one reflection at either end must land inside [0, n_total) */
        if (p.B < 1 || p.B > 65535 || !dim(p.T) || p.n_total <= TK_WH_NFFT / 2 || p.n_total > (1 << 24) || p.n_samples < 1 || p.n_samples > p.n_total || p.pcm_stride < p.n_samples ||
            p.pcm_stride > (1 << 24))
            return false;
        const int64_t last = ((int64_t)p.T - 1) * TK_WH_HOP + TK_WH_NFFT - 1 - TK_WH_NFFT / 2;
        if (last > 2 * ((int64_t)p.n_total - 1)) return false;
        o.a = ((int64_t)p.B - 1) * p.pcm_stride + p.n_samples; o.sa = 2;
        o.b = TK_WH_NFFT;
        o.y = (int64_t)p.B * p.T * TK_WH_NFFT;
        return o.a <= big && o.y <= big;
    }
    case TK_MI355X_EDGE_POWER:
        if (!dim(p.rows) || !dim(p.nb) || (int64_t)p.rows * p.nb * 2 > big) return false;
        o.a = (int64_t)p.rows * p.nb * 2; o.y = (int64_t)p.rows * p.nb;
        return true;
    case TK_MI355X_EDGE_LOGMEL_FINISH:
        if (p.B < 1 || p.B > 65535 || !dim(p.per_b) || (int64_t)p.B * p.per_b > big) return false;
        o.y = (int64_t)p.B * p.per_b;
        return true;
    case TK_MI355X_EDGE_VAD_HEAD:
        if (!dim(p.rows) || !dim(p.hidden) || (int64_t)p.rows * p.hidden > big) return false;
        o.a = (int64_t)p.rows * p.hidden; o.b = p.hidden; o.c = 1; o.y = p.rows;
        return true;
    case TK_MI355X_EDGE_PREPROCESS: {
        if (p.in_w < 2 || p.in_w > cap || p.in_h < 2 || p.in_h > cap || !dim(p.out_w) || p.out_h < 1 || p.out_h > (1 << 18) || (p.bpp != 3 && p.bpp != 4) || (p.nhwc != 0 && p.nhwc != 1) ||
            p.in_stride < (int64_t)p.in_w * p.bpp || p.in_stride > (1 << 24) || !finite(p.scale))
            return false;
        /* the last tap: row in_h - 1, pixel in_w - 1, channel 2 */
        o.a = ((int64_t)p.in_h - 1) * p.in_stride + ((int64_t)p.in_w - 1) * p.bpp + 3; o.sa = 1;
        o.y = 3 * (int64_t)p.out_w * p.out_h;
        return o.a <= big && o.y <= big;
    }
    case TK_MI355X_EDGE_DEPTH_MINMAX:
    case TK_MI355X_EDGE_DEPTH_METRIC:
        if (p.n < 1 || p.n > big) return false;
        o.a = p.n;
        if (p.op == TK_MI355X_EDGE_DEPTH_MINMAX) o.y = 2;
        else { o.y = p.n; o.y2 = 2; }
        return true;
    case TK_MI355X_EDGE_POSTPROCESS_DEPTH:
    case TK_MI355X_EDGE_DEPTH_TO_POINTS: {
        if (!dim(p.width) || !dim(p.height) || (int64_t)p.width * p.height * 3 > big) return false;
        const int64_t n = (int64_t)p.width * p.height;
        o.a = n;
        o.y = p.op == TK_MI355X_EDGE_DEPTH_TO_POINTS ? 3 * n : n;
        return true;
    }
    case TK_MI355X_EDGE_BOX_ATTRIBUTES:
        if (!dim(p.in_w) || !dim(p.in_h) || !dim(p.rows) || (int64_t)p.in_w * p.in_h * 3 > big) return false;
        o.a = (int64_t)p.in_w * p.in_h * 3; o.sa = 1;
        o.b = 4 * (int64_t)p.rows;
        o.y = 2 * (int64_t)p.rows;
        return true;
    default: return false;
    }
}

/* the launch itself (or, with dry, the launcher's answer alone) on the given bases; false: the launcher refuses */
static bool edge_probe_launch(tk_mi355x_edge_probe_t& p, const void* a, const void* b, const void* c, void* y, void* y2, bool dry) {
    p.kernel = 0;
    switch (p.op) {
    case TK_MI355X_EDGE_FRAMES:
        if (!dry) tk_launch_frames((const int16_t*)a, p.B, p.n_samples, p.pcm_stride, p.n_total, p.T, (const float*)b, (float*)y, nullptr);
        return true;
    case TK_MI355X_EDGE_POWER:
        if (!dry) tk_launch_power((const float*)a, p.rows, p.nb, (float*)y, nullptr);
        return true;
    case TK_MI355X_EDGE_LOGMEL_FINISH:
        if (!dry) tk_launch_logmel_finish((float*)y, p.B, p.per_b, nullptr);
        return true;
    case TK_MI355X_EDGE_VAD_HEAD:
        if (!dry) tk_launch_vad_head((const float*)a, p.rows, p.hidden, (const float*)b, (const float*)c, (float*)y, nullptr);
        return true;
    case TK_MI355X_EDGE_PREPROCESS: {
        TkPreprocessArgs g{};
        g.src = (const uint8_t*)a; g.in_w = (uint32_t)p.in_w; g.in_h = (uint32_t)p.in_h; g.in_stride = (uint32_t)p.in_stride; g.bpp = (uint32_t)p.bpp;
        g.dst = (float*)y; g.out_w = (uint32_t)p.out_w; g.out_h = (uint32_t)p.out_h; g.nhwc = p.nhwc;
        for (int i = 0; i < 3; ++i) { g.mean[i] = p.mean[i]; g.std_dev[i] = p.std_dev[i]; }
        p.kernel = launch_preprocess_for_scale(g, p.scale, nullptr, dry);
        return true;
    }
    case TK_MI355X_EDGE_DEPTH_MINMAX:
        if (!dry) tk_launch_depth_minmax((const float*)a, p.n, (float*)y, nullptr);
        return true;
    case TK_MI355X_EDGE_DEPTH_METRIC: /* as TkDepthEngine::to_metric: the two launches in stream order */
        if (!dry) {
            tk_launch_depth_minmax((const float*)a, p.n, (float*)y2, nullptr);
            tk_launch_depth_metric((const float*)a, (const float*)y2, p.min_depth, p.max_depth, (float*)y, p.n, nullptr);
        }
        return true;
    case TK_MI355X_EDGE_POSTPROCESS_DEPTH: {
        const tk_postprocess_depth_params_t q{(const float*)a, (uint32_t)p.width, (uint32_t)p.height, (float*)y, p.scale, p.shift};
        p.kernel = (int32_t)depth_grid_blocks((size_t)p.width * p.height);
        return dry || tk_kernels_postprocess_depth_map(&q, nullptr) == TK_SUCCESS;
    }
    case TK_MI355X_EDGE_DEPTH_TO_POINTS: {
        const tk_depth_to_points_params_t q{(const float*)a, (uint32_t)p.width, (uint32_t)p.height, (tk_float3*)y, p.fx, p.fy, p.cx, p.cy};
        p.kernel = (int32_t)depth_grid_blocks((size_t)p.width * p.height);
        if (p.fx == 0.0f || p.fy == 0.0f) { p.kernel = -1; return false; } /* the launcher's own refusal */
        return dry || tk_kernels_depth_to_point_cloud(&q, nullptr) == TK_SUCCESS;
    }
    case TK_MI355X_EDGE_BOX_ATTRIBUTES:
        if (!dry) tk_launch_box_attributes((const uint8_t*)a, p.in_w, p.in_h, p.rows, (const int32_t*)b, (int32_t*)y, nullptr);
        return true;
    default: return false;
    }
}

tk_error_code_t tk_mi355x_edge_probe(int device, tk_mi355x_edge_probe_t* p) {
    static_assert(sizeof(tk_float3) == 12, "a point is three packed floats");
    if (!p) return TK_ERROR_INVALID_ARGUMENT;
    p->kernel = -1;
    EdgeReach need;
    if (!edge_probe_reach(*p, need)) return TK_ERROR_INVALID_ARGUMENT;
    /* an array the op uses must be there and long enough; one it does not use must be absent */
    auto fits = [](const void* ptr, int64_t n, int64_t want) { return want == 0 ? (ptr == nullptr && n == 0) : (ptr != nullptr && n >= want); };
    if (!fits(p->a, p->n_a, need.a) || !fits(p->b, p->n_b, need.b) || !fits(p->c, p->n_c, need.c) || !fits(p->y, p->n_y, need.y) || !fits(p->y2, p->n_y2, need.y2))
        return TK_ERROR_INVALID_ARGUMENT;
    if (p->op == TK_MI355X_EDGE_BOX_ATTRIBUTES) { /* a test hook: boxes a launch walks in no time (the public entry points take any rectangle, ABI_NOTES.md) */
        const int32_t* r = (const int32_t*)p->b;
        const int32_t far = 1 << 30, wide = 1 << 20;
        for (int i = 0; i < p->rows; ++i) {
            const int32_t bx = r[4 * i], by = r[4 * i + 1], bw = r[4 * i + 2], bh = r[4 * i + 3];
            if (bx < -far || bx > far || by < -far || by > far || bw < -wide || bw > wide || bh < -wide || bh > wide) return TK_ERROR_INVALID_ARGUMENT;
            if (bw > 0 && bh > 0 && (int64_t)bw * bh > ((int64_t)1 << 24)) return TK_ERROR_INVALID_ARGUMENT;
        }
    }
    if (device < 0) {
        const void* aligned = (const void*)(uintptr_t)256;
        return edge_probe_launch(*p, aligned, aligned, aligned, (void*)(uintptr_t)256, (void*)(uintptr_t)256, true) ? TK_SUCCESS : TK_ERROR_INVALID_ARGUMENT;
    }
    { tk_mi355x_edge_probe_t dry = *p; /* what the launcher refuses is refused before the device is touched */
      if (!edge_probe_launch(dry, p->a, p->b, p->c, p->y, p->y2, true)) { p->kernel = dry.kernel; return TK_ERROR_INVALID_ARGUMENT; } }
    tk_error_code_t rc = probe_device(device);
    if (rc != TK_SUCCESS) return rc;
    enum { A, Bm, Cm, Y, Y2, NBUF };
    ProbeBuf b[NBUF] = {{p->a, (size_t)p->n_a * need.sa, 0, false, nullptr}, {p->b, (size_t)p->n_b * need.sb, 0, false, nullptr},
                        {p->c, (size_t)p->n_c * 4, 0, false, nullptr}, {p->y, (size_t)p->n_y * need.sy, 0, true, nullptr},
                        {p->y2, (size_t)p->n_y2 * 4, 0, true, nullptr}};
    if (!probe_upload(b, NBUF)) rc = TK_ERROR_GPU_ROCM_ERROR;
    else {
        if (!edge_probe_launch(*p, b[A].dev, b[Bm].dev, b[Cm].dev, b[Y].dev, b[Y2].dev, false)) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || !probe_download(b, NBUF)) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    probe_free(b, NBUF);
    return rc;
}

tk_error_code_t tk_mi355x_detector_post_probe(int device, tk_mi355x_detector_post_probe_t* p) {
    static_assert(sizeof(tk_mi355x_box_t) == sizeof(tk_yolo_cand_t) && sizeof(tk_mi355x_box_t) == sizeof(TkDetection), "the public record is the kernels' candidate and detection");
    if (!p || (p->kind != 0 && p->kind != 1) || p->B < 1 || p->B > 256 || p->nc < 1 || p->nc > 4096 || p->n_anchors < 1 || p->n_anchors > (1 << 20))
        return TK_ERROR_INVALID_ARGUMENT;
    const int64_t B = p->B, words = TK_YOLO_MAX_CAND / 64;
    TkT heads[3];
    if (p->kind == 0) {
        if (p->in_w < 32 || p->in_h < 32 || p->in_w > 4096 || p->in_h > 4096 || (p->in_w & 31) || (p->in_h & 31) || p->out || p->n_out != 0) return TK_ERROR_INVALID_ARGUMENT;
        int64_t total = 0;
        for (int i = 0; i < 3; ++i) {
            const int H = p->in_h >> (3 + i), W = p->in_w >> (3 + i);
            if (!p->head[i] || p->ld[i] < 64 + p->nc || p->ld[i] > (1 << 16) || p->n_head[i] < (B * H * W - 1) * p->ld[i] + 64 + p->nc) return TK_ERROR_INVALID_ARGUMENT;
            heads[i].B = p->B; heads[i].H = H; heads[i].W = W; heads[i].C = 64 + p->nc; heads[i].ld = p->ld[i];
            total += (int64_t)H * W;
        }
        if (total != p->n_anchors) return TK_ERROR_INVALID_ARGUMENT;
    } else {
        if (!p->out || p->n_out < B * (4 + p->nc) * p->n_anchors) return TK_ERROR_INVALID_ARGUMENT;
        for (int i = 0; i < 3; ++i) if (p->head[i] || p->n_head[i] != 0) return TK_ERROR_INVALID_ARGUMENT;
    }
    if (!p->cand || !p->order || !p->n_cand || !p->kept || !p->n_kept || p->cand_count != B * p->n_anchors || p->order_count != B * TK_YOLO_MAX_CAND ||
        p->n_cand_count != B || p->kept_count != B * TK_OBJECT_DETECTOR_MAX_DETECTIONS || p->n_kept_count != B ||
        (p->mask ? p->mask_count != B * TK_YOLO_MAX_CAND * words : p->mask_count != 0))
        return TK_ERROR_INVALID_ARGUMENT;
    if (device < 0) return TK_SUCCESS;
    tk_error_code_t rc = probe_device(device);
    if (rc != TK_SUCCESS) return rc;
    enum { H0, H1, H2, OUT, CAND, ORDER, NCAND, MASK, KEPT, NKEPT, NBUF };
    const size_t rec = sizeof(tk_mi355x_box_t);
    ProbeBuf b[NBUF] = {{p->head[0], (size_t)p->n_head[0] * 4, 0, false, nullptr}, {p->head[1], (size_t)p->n_head[1] * 4, 0, false, nullptr},
                        {p->head[2], (size_t)p->n_head[2] * 4, 0, false, nullptr}, {p->out, (size_t)p->n_out * 4, 0, false, nullptr},
                        {p->cand, (size_t)p->cand_count * rec, 0, true, nullptr}, {p->order, (size_t)p->order_count * 4, 0, true, nullptr},
                        {p->n_cand, (size_t)B * 4, 0, true, nullptr}, {p->mask, (size_t)p->mask_count * 8, 0, true, nullptr},
                        {p->kept, (size_t)p->kept_count * rec, 0, true, nullptr}, {p->n_kept, (size_t)B * 4, 0, true, nullptr}};
    void* own_mask = nullptr; /* no host mask: the matrix still exists on the device, stale like the caller's other arrays */
    const size_t mask_bytes = (size_t)B * TK_YOLO_MAX_CAND * words * 8;
    bool ok = probe_upload(b, NBUF);
    if (ok && !p->mask) ok = hipMalloc(&own_mask, mask_bytes) == hipSuccess && hipMemset(own_mask, 0xFF, mask_bytes) == hipSuccess;
    if (!ok) rc = TK_ERROR_GPU_ROCM_ERROR;
    else {
        tk_yolo_cand_t* cand = (tk_yolo_cand_t*)b[CAND].dev;
        bool launched = true;
        if (p->kind == 0) {
            for (int i = 0; i < 3; ++i) heads[i].p = (float*)b[H0 + i].dev;
            launched = tk_launch_yolo_decode(heads, p->B, p->nc, p->n_anchors, p->conf, cand, nullptr);
        } else
            for (int f = 0; f < p->B && launched; ++f)
                launched = tk_launch_yolo_decode_out((const float*)b[OUT].dev + (size_t)f * (4 + p->nc) * p->n_anchors, p->nc, p->n_anchors, p->conf,
                                                     cand + (size_t)f * p->n_anchors, nullptr);
        launched = launched && tk_launch_yolo_post(cand, p->n_anchors, p->B, p->iou, (int32_t*)b[ORDER].dev, (int32_t*)b[NCAND].dev,
                                                   (uint64_t*)(p->mask ? b[MASK].dev : own_mask), (TkDetection*)b[KEPT].dev, (int32_t*)b[NKEPT].dev, nullptr);
        if (!launched) rc = TK_ERROR_INVALID_ARGUMENT;
        else if (hipGetLastError() != hipSuccess) rc = TK_ERROR_GPU_KERNEL_LAUNCH;
        else if (hipDeviceSynchronize() != hipSuccess || !probe_download(b, NBUF)) rc = TK_ERROR_GPU_ROCM_ERROR;
    }
    probe_free(b, NBUF);
    if (own_mask) (void)hipFree(own_mask);
    return rc;
}

tk_error_code_t tk_kernels_depth_to_point_cloud(const tk_depth_to_points_params_t* p, tk_hip_stream_t stream) {
    if (!p || !p->d_metric_depth_map || !p->d_point_cloud || p->width == 0 || p->height == 0 || p->fx == 0.0f || p->fy == 0.0f)
        return TK_ERROR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(k_depth_to_points, dim3(depth_grid_blocks((size_t)p->width * p->height)), dim3(256), 0, (hipStream_t)stream, *p);
    return launch_status();
}

tk_error_code_t tk_rocm_dispatch_create(tk_rocm_dispatcher_t** out, const tk_rocm_dispatcher_config_t* config) {
    if (!out || !config) return TK_ERROR_INVALID_ARGUMENT;
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return TK_ERROR_GPU_DEVICE_NOT_FOUND;
    if (config->device_id < 0 || config->device_id >= n) return TK_ERROR_INVALID_ARGUMENT;
    tk_rocm_dispatcher_s* d = (tk_rocm_dispatcher_s*)calloc(1, sizeof *d);
    if (!d) return TK_ERROR_OUT_OF_MEMORY;
    d->device = config->device_id;
    if (hipSetDevice(d->device) != hipSuccess || hipStreamCreateWithFlags(&d->compute, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&d->h2d, hipStreamNonBlocking) != hipSuccess || hipStreamCreateWithFlags(&d->d2h, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_upload, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&d->ev_compute, hipEventDisableTiming) != hipSuccess) {
        free(d);
        return TK_ERROR_GPU_ROCM_ERROR;
    }
    *out = d;
    return TK_SUCCESS;
}

void tk_rocm_dispatch_destroy(tk_rocm_dispatcher_t** dispatcher) {
    if (!dispatcher || !*dispatcher) return;
    tk_rocm_dispatcher_s* d = *dispatcher;
    (void)hipSetDevice(d->device);
    (void)hipDeviceSynchronize();
    (void)hipStreamDestroy(d->compute); (void)hipStreamDestroy(d->h2d); (void)hipStreamDestroy(d->d2h);
    (void)hipEventDestroy(d->ev_upload); (void)hipEventDestroy(d->ev_compute);
    free(d);
    *dispatcher = NULL;
}

tk_error_code_t tk_rocm_dispatch_malloc(tk_rocm_dispatcher_t* d, tk_gpu_buffer_t* out_buffer, size_t size_bytes) {
    if (!d || !out_buffer || size_bytes == 0) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    tk_gpu_buffer_s* b = (tk_gpu_buffer_s*)calloc(1, sizeof *b);
    if (!b) return TK_ERROR_OUT_OF_MEMORY;
    if (hipMalloc(&b->dptr, size_bytes) != hipSuccess) { free(b); return TK_ERROR_GPU_MEMORY; }
    b->size = size_bytes;
    *out_buffer = b;
    return TK_SUCCESS;
}

void tk_rocm_dispatch_free(tk_rocm_dispatcher_t* d, tk_gpu_buffer_t* buffer) {
    if (!d || !buffer || !*buffer) return;
    (void)hipSetDevice(d->device);
    (void)hipFree((*buffer)->dptr);
    free(*buffer);
    *buffer = NULL;
}

void* tk_rocm_dispatch_buffer_ptr(tk_gpu_buffer_t buffer) { return buffer ? buffer->dptr : NULL; }

tk_error_code_t tk_rocm_dispatch_upload_async(tk_rocm_dispatcher_t* d, tk_gpu_buffer_t dst, const void* src, size_t n) {
    if (!d || !dst || !src || n > dst->size) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    if (hipMemcpyAsync(dst->dptr, src, n, hipMemcpyHostToDevice, d->h2d) != hipSuccess) return TK_ERROR_GPU_MEMORY;
    /* kernels enqueued afterwards must see the data */
    if (hipEventRecord(d->ev_upload, d->h2d) != hipSuccess || hipStreamWaitEvent(d->compute, d->ev_upload, 0) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    return TK_SUCCESS;
}

tk_error_code_t tk_rocm_dispatch_download_async(tk_rocm_dispatcher_t* d, void* dst, tk_gpu_buffer_t src, size_t n) {
    if (!d || !dst || !src || n > src->size) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    if (hipEventRecord(d->ev_compute, d->compute) != hipSuccess || hipStreamWaitEvent(d->d2h, d->ev_compute, 0) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    if (hipMemcpyAsync(dst, src->dptr, n, hipMemcpyDeviceToHost, d->d2h) != hipSuccess) return TK_ERROR_GPU_MEMORY;
    return TK_SUCCESS;
}

tk_error_code_t tk_rocm_dispatch_synchronize(tk_rocm_dispatcher_t* d) {
    if (!d) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    if (hipStreamSynchronize(d->h2d) != hipSuccess || hipStreamSynchronize(d->compute) != hipSuccess || hipStreamSynchronize(d->d2h) != hipSuccess)
        return TK_ERROR_GPU_ROCM_ERROR;
    return TK_SUCCESS;
}

tk_error_code_t tk_rocm_dispatch_get_stream(tk_rocm_dispatcher_t* d, tk_hip_stream_t* stream) {
    if (!d || !stream) return TK_ERROR_INVALID_ARGUMENT;
    *stream = (tk_hip_stream_t)d->compute;
    return TK_SUCCESS;
}

tk_error_code_t tk_rocm_dispatch_preprocess_image(tk_rocm_dispatcher_t* d, const tk_preprocess_params_t* params) {
    if (!d) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    return tk_kernels_preprocess_image(params, (tk_hip_stream_t)d->compute);
}

tk_error_code_t tk_rocm_dispatch_depth_to_point_cloud(tk_rocm_dispatcher_t* d, const tk_depth_to_points_params_t* params) {
    if (!d) return TK_ERROR_INVALID_ARGUMENT;
    if (hipSetDevice(d->device) != hipSuccess) return TK_ERROR_GPU_ROCM_ERROR;
    return tk_kernels_depth_to_point_cloud(params, (tk_hip_stream_t)d->compute);
}

} /* extern "C" */
