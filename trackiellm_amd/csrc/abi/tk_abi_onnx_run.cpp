/*
 * tk_abi_onnx_run.cpp — tk_mi355x_onnx_run (include/tk/tk_mi355x_ext.h): one small ONNX graph on arbitrary float tensors through the
 * node-by-node executor, for the per-op tests (tests/test_onnx_ops_gpu.py).  Everything lives for one call: a stream, the executor, the
 * device copies of the feeds.
 */
#include <hip/hip_runtime.h>

#include <memory>
#include <string>
#include <vector>

#include "../nn/tk_onnx_exec.h"
#include "tk/tk_error_handling.h"
#include "tk/tk_mi355x_ext.h"

struct tk_mi355x_onnx_result_s {
    std::vector<std::vector<int64_t>> dims;
    std::vector<std::vector<float>> data;
};

namespace {
tk_error_code_t ofail(tk_error_code_t code, const std::string& why) {
    tk_error_set_detail("%s", why.c_str());
    return code;
}

struct RunScope { /* frees in the right order: the executor waits for the stream before the stream goes */
    TkOnnxExec exec;
    hipStream_t stream = nullptr;
    std::vector<float*> feeds;
    ~RunScope() {
        exec.unload();
        for (float* p : feeds) if (p) (void)hipFree(p);
        if (stream) (void)hipStreamDestroy(stream);
    }
};
}  // namespace

extern "C" {

tk_error_code_t tk_mi355x_onnx_run(int device, const char* path, int32_t n_feeds, const char* const* feed_names, const float* const* feed_data,
                                   const int32_t* feed_ranks, const int64_t* const* feed_dims, int32_t n_outputs, const char* const* output_names,
                                   tk_mi355x_onnx_result_t** out_result) {
    if (!path || !out_result || n_feeds < 0 || n_outputs < 1 || !output_names || (n_feeds > 0 && (!feed_names || !feed_data || !feed_ranks || !feed_dims)))
        return TK_ERROR_INVALID_ARGUMENT;
    *out_result = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) return ofail(TK_ERROR_GPU_DEVICE_NOT_FOUND, "no HIP device visible");
    if (device < 0 || device >= ndev || hipSetDevice(device) != hipSuccess) return ofail(TK_ERROR_INVALID_ARGUMENT, "device out of range");
    try {
        RunScope s;
        if (hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking) != hipSuccess) return ofail(TK_ERROR_GPU_ROCM_ERROR, "hipStreamCreate failed");
        if (!s.exec.load(path, device, s.stream, (size_t)1 << 24)) return ofail(TK_ERROR_MODEL_LOAD_FAILED, s.exec.error); /* 64 MiB of activations */
        for (int32_t i = 0; i < n_feeds; ++i) {
            if (!feed_names[i] || !feed_data[i] || feed_ranks[i] < 0 || feed_ranks[i] > 8 || (feed_ranks[i] > 0 && !feed_dims[i])) return ofail(TK_ERROR_INVALID_ARGUMENT, "bad feed");
            TkOnnxExec::Val v;
            for (int32_t d = 0; d < feed_ranks[i]; ++d) {
                if (feed_dims[i][d] < 0 || feed_dims[i][d] > (1 << 24)) return ofail(TK_ERROR_INVALID_ARGUMENT, "bad feed dimension");
                v.shape.push_back(feed_dims[i][d]);
            }
            const int64_t n = v.count();
            if (n > (1 << 24)) return ofail(TK_ERROR_INVALID_ARGUMENT, "feed too large");
            float* d = nullptr;
            if (hipMalloc((void**)&d, (size_t)(n > 0 ? n : 1) * 4) != hipSuccess) return ofail(TK_ERROR_OUT_OF_MEMORY, "hipMalloc failed");
            s.feeds.push_back(d);
            if (n > 0 && hipMemcpy(d, feed_data[i], (size_t)n * 4, hipMemcpyHostToDevice) != hipSuccess) return ofail(TK_ERROR_GPU_ROCM_ERROR, "upload failed");
            v.d = d;
            s.exec.bind(feed_names[i], v);
        }
        if (!s.exec.run()) return ofail(TK_ERROR_INFERENCE_FAILED, s.exec.error);
        if (hipStreamSynchronize(s.stream) != hipSuccess) return ofail(TK_ERROR_GPU_ROCM_ERROR, "the graph's kernels failed");
        std::unique_ptr<tk_mi355x_onnx_result_s> r(new tk_mi355x_onnx_result_s());
        for (int32_t i = 0; i < n_outputs; ++i) {
            const TkOnnxExec::Val* o = output_names[i] ? s.exec.value(output_names[i]) : nullptr;
            if (!o) return ofail(TK_ERROR_INFERENCE_FAILED, std::string("the graph produced no value named '") + (output_names[i] ? output_names[i] : "") + "'");
            if (o->is_int || !o->d) return ofail(TK_ERROR_INFERENCE_FAILED, std::string("value '") + output_names[i] + "' is an integer tensor");
            const int64_t n = o->count();
            std::vector<float> host((size_t)(n > 0 ? n : 0));
            if (n > 0 && hipMemcpy(host.data(), o->d, (size_t)n * 4, hipMemcpyDeviceToHost) != hipSuccess) return ofail(TK_ERROR_GPU_ROCM_ERROR, "download failed");
            r->dims.push_back(o->shape);
            r->data.push_back(std::move(host));
        }
        *out_result = r.release();
        return TK_SUCCESS;
    } catch (const std::exception& ex) { return ofail(TK_ERROR_MODEL_LOAD_FAILED, ex.what()); }
}

int32_t tk_mi355x_onnx_result_rank(const tk_mi355x_onnx_result_t* r, int32_t i) {
    return (!r || i < 0 || (size_t)i >= r->dims.size()) ? -1 : (int32_t)r->dims[(size_t)i].size();
}

const int64_t* tk_mi355x_onnx_result_dims(const tk_mi355x_onnx_result_t* r, int32_t i) {
    return (!r || i < 0 || (size_t)i >= r->dims.size()) ? nullptr : r->dims[(size_t)i].data();
}

const float* tk_mi355x_onnx_result_data(const tk_mi355x_onnx_result_t* r, int32_t i) {
    return (!r || i < 0 || (size_t)i >= r->data.size()) ? nullptr : r->data[(size_t)i].data();
}

void tk_mi355x_onnx_result_free(tk_mi355x_onnx_result_t** r) {
    if (!r || !*r) return;
    delete *r;
    *r = nullptr;
}

} /* extern "C" */
