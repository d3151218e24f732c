/*
 * tk_nn_kernels.h — fp32 building blocks shared by the detector and ASR streams.
 *
 * The reference runs these networks inside ONNX Runtime / whisper.cpp (absent: SURVEY.md §0 F1).
 * Here every dense contraction (conv as implicit GEMM, linear layers, QK^T, PV, the DFT and
 * mel filterbank) goes through ONE kernel, tk_gemm_f32, built on v_mfma_f32_32x32x2_f32.
 * That instruction is bit-for-bit a k-ordered fp32 fma chain, so with the accumulator started at
 * zero and k walked in ascending order the result equals the oracle's
 *     acc = 0; for k: acc = fmaf(a[k], b[k], acc);  out = act(acc + bias) (+ residual)
 * exactly — the detector and ASR parity tests are 0-ulp, like the LLM ones.
 * fp32 (not bf16) is deliberate: YOLOv8n is 8.7 GFLOP and the Whisper-tiny encoder 37 GFLOP per
 * call, ~1 ms of fp32 MFMA against a >= 70 ms LLM decode; exactness is worth more than speed here.
 */
#ifndef TK_NN_KERNELS_H
#define TK_NN_KERNELS_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../common/tk_gemm_desc.h"

/* false (nothing launched): a descriptor tk_gemm_kernel_of refuses — one without output cells (M < 1 or N < 1: nothing is left stale), or an
 * implicit-im2col form outside tk_gemm_im2col_ok().  The engines' callers drop the result because they cannot be refused: im_* is set in one
 * place only (the detector's conv, csrc/vision/tk_vision_engine.hip), after tk_gemm_im2col_ok() held for its input and [N][K] f32 weights, with
 * b_kn = 0 and ldb = K = k k C, C % 4 == 0; every other caller leaves im_C = 0, for which only an empty extent is refused.  A caller that builds
 * descriptors from outside data (the test hook tk_mi355x_gemm_probe) checks the result. */
bool tk_launch_gemm(const TkGemm& g, hipStream_t s);
/* which kernel and instantiation tk_launch_gemm takes for g — a pure host function, and the launcher's own switch:
 * code = family * 1000 + IM * 100 + PATH * 10 + NT (IM: implicit im2col; PATH: the operand loaders' instantiation, 0 element-wise fallbacks,
 * 1 [N][K] and 2 [K][N] 16-byte groups; NT: 32-column accumulators per wave of the tall kernels, 0 elsewhere), or TK_GEMM_REFUSED */
enum { TK_GEMM_F32 = 0, TK_GEMM_F32_TALL = 1, TK_GEMM_F32_BIG = 2, TK_GEMM_H3_TALL = 3, TK_GEMM_H3_BIG = 4, TK_GEMM_REFUSED = -1 };
#define TK_GEMM_CODE(FAMILY, IM, PATH, NT) ((FAMILY) * 1000 + ((IM) ? 100 : 0) + (PATH) * 10 + (NT))
#define TK_GEMM_FAMILY(CODE) ((CODE) / 1000)
int tk_gemm_kernel_of(const TkGemm& g);
/* whether a convolution can be addressed by the GEMM itself (TkGemm::im_*): channels and pitch multiples of 4, input x and the [N][K]
 * f32 weights w 16-byte aligned */
bool tk_gemm_im2col_ok(const float* x, int C, int ldx, const float* w);
/* direct 3x3 convolution of a 3-channel image into 16 channels (the detector's stem), the GEMM's chain and epilogue (bias, act) per
 * output; false (nothing launched): another shape — use im2col + tk_launch_gemm */
/* the stem launcher's admission test, a pure host function: N == 16, C == 3, k == 3, ldy % 4 == 0, y 16-byte aligned, a non-empty output of
 * fewer than 2^31 pixels, stride >= 1, pad >= 0, pitches not below the extents */
bool tk_conv_stem_ok(int B, int H, int W, int C, int ldx, int N, int k, int stride, int pad, const float* y, int ldy);
bool tk_launch_conv_stem(const float* x, int B, int H, int W, int C, int ldx, const float* w, const float* bias, int act, int N, int k, int stride, int pad, float* y,
                         int ldy, hipStream_t s);
/* opts the large-tile GEMM into its dynamic LDS on the calling thread's current device; idempotent, thread-safe.  tk_launch_gemm does
 * it on first use; callers that capture launches into a hipGraph call it beforehand. */
bool tk_nn_prepare_device();
/* opt-in (the fast contraction's companion, TkGemm::fast): attention over Tk keys for Tq queries per (sequence, head) in ONE kernel — Q K^T, online
 * softmax, P V on the f16 matrix pipe with split operands, no score matrix in HBM; head_dim 64, q / k / v / out rows of pitch d = nh * 64,
 * 16-byte aligned.  false (nothing launched): another geometry.  ~1e-6 of scale off the exact three-launch form, not its bits. */
bool tk_launch_attention_h3(const float* q, const float* k, const float* v, float* out, int B, int nh, int Tq, int Tk, int64_t q_bstride, int64_t kv_bstride, int d,
                            float scale, hipStream_t s);

/* The row and layout launchers below return false with nothing launched for what no caller sends: an empty extent (rows, B, H, W, C, D < 1),
 * a pitch below the extent, a stride < 1, a negative pad, a window wider than the padded input, more 256-element blocks than a grid holds.
 * Every caller checks the result: the engines report a refusal as their own error, the hooks as TK_ERROR_INVALID_ARGUMENT. */
/* NHWC im2col: col[b*Ho*Wo + oy*Wo + ox][(ky*kw + kx)*C + c]; input row stride ldx floats per pixel */
[[nodiscard]] bool tk_launch_im2col(const float* x, int B, int H, int W, int C, int ldx, int kh, int kw, int stride, int pad, float* col, hipStream_t s);
/* which kernel tk_launch_im2col takes — a pure host function and the launcher's own switch: the 16-byte kernel needs C % 4 == 0, ldx % 4 == 0,
 * x and col 16-byte aligned and fewer than 2^31 groups */
enum { TK_IM2COL_ELEMENT = 0, TK_IM2COL_V4 = 1, TK_IM2COL_REFUSED = -1 };
int tk_im2col_kernel_of(const float* x, int B, int H, int W, int C, int ldx, int kh, int kw, int stride, int pad, const float* col);
[[nodiscard]] bool tk_launch_maxpool5(const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, hipStream_t s);
[[nodiscard]] bool tk_launch_upsample2x(const float* x, int B, int H, int W, int C, int ldx, float* y, int ldy, hipStream_t s);
[[nodiscard]] bool tk_launch_copy_cols(const float* x, int rows, int C, int ldx, float* y, int ldy, hipStream_t s);
/* rows of [T][C] (row pitch ldx) -> col[b*To + t][(kx*C + c)], kernel width kw, zero padding `pad` on both ends */
[[nodiscard]] bool tk_launch_im2col1d(const float* x, int B, int T, int C, int ldx, int kw, int stride, int pad, float* col, hipStream_t s);
/* out[r][:] = table[idx[r]][:] + pos[(pos0[r])][:] */
[[nodiscard]] bool tk_launch_embed_rows(const float* table, const float* pos, const int32_t* idx, const int32_t* pos_idx, int rows, int D, float* out, hipStream_t s);
void tk_launch_argmax_rows(const float* x, int rows, int cols, int ld, int32_t* out, hipStream_t s);
/* Whisper's language detection (common/tk_lang_pick.h) over the n_lang logits from column tok0 on of every row: lang_id [rows], prob_id [rows] =
 * the probability of the row's language, probs (optional) [rows][n_lang]; where auto_row[row] != 0 the token tok0 + id is stored into slot[row]
 * (both optional; other rows' slots stay untouched).  false, nothing launched: a geometry tk_lang_pick_check refuses */
[[nodiscard]] bool tk_launch_lang_pick(const float* x, int rows, int cols, int ld, int tok0, int n_lang, const int32_t* auto_row, int32_t* slot, int32_t* lang_id,
                                       float* prob_id, float* probs, hipStream_t s);
/* token pick under whisper.cpp's decoding policy: arg max (temp 0) or one draw from softmax(l / temp), + the pick's log-probability under
 * that distribution per row (logprob may be null); the generator is keyed by (seed, counter0 + row) */
struct TkPick { float temp; uint64_t seed; uint32_t counter0; float* logprob; };
void tk_launch_pick_rows(const float* x, int rows, int cols, int ld, int32_t* out, const TkPick& pk, hipStream_t s);
/* whisper.cpp's whisper_process_logits + the per-token bookkeeping of whisper_full's decode loop, as the reference's wrapper configures them
 * (src/audio/tk_asr_whisper.c:89-110: suppress_blank off, suppress_non_speech_tokens on, timestamps on, max_initial_ts at its default 1.0 s):
 * per row a static suppression table, the timestamp rules (pairs, initial cap, monotonic), "timestamps win when their summed probability beats
 * every text token", then the pick (arg max or one draw) and its log-probability, then the row's decode state moves on.
 * state[row][8] = {tokens sampled, last was a timestamp, the one before was, has_ts, seek_delta, result_len, status (0 running, 1 completed,
 * 2 failed), seek_end (10 ms frames of the utterance)}; a row whose status is not 0 emits `eot` and stands still. */
#define TK_WH_STATE_INTS 8
struct TkWhFilter { const uint8_t* suppress; int32_t* state; int32_t beg, eot, tid0; };
void tk_launch_pick_rows_filtered(const float* x, int rows, int cols, int ld, int32_t* out, const TkPick& pk, const TkWhFilter& f, hipStream_t s);
/* also refused: an image with D % 16 != 0 (its 16-row blocks would overlap) */
[[nodiscard]] bool tk_launch_layernorm(const float* x, int rows, int D, const float* w, const float* b, float eps, float* y, hipStream_t s, float* img = nullptr /* optional: also the tiled GEMM's operand image of y */);
[[nodiscard]] bool tk_launch_softmax_rows(float* x, int rows, int cols, int ld, hipStream_t s);
/* which of the three bit-identical kernels tk_launch_softmax_rows takes — a pure host function and the launcher's own switch: one wave per row
 * (cols <= 2048, cols and ld multiples of 4, base 16-byte aligned, rows >= 1024), one block per row out of registers (cols <= 2048), or the
 * three-pass kernel */
enum { TK_SOFTMAX_GENERIC = 0, TK_SOFTMAX_REG = 1, TK_SOFTMAX_WAVE = 2, TK_SOFTMAX_REFUSED = -1 };
int tk_softmax_kernel_of(int rows, int cols, int ld, const float* base);
[[nodiscard]] bool tk_launch_add_rows(float* x, const float* add, int rows, int D, int add_rows, hipStream_t s);

#endif
