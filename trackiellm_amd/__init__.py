"""trackiellm_amd — Python host-side mirror of the tk_* C-ABI of libtrackie_mi355x.so.

The product is the shared library (hand-written gfx950 HIP kernels behind TrackieLLM's own
C operator surface).  This package only binds it with ctypes so that tests, bench.py and
Python callers can drive exactly the entry points a C/Rust host would link against.
There is no Python or CPU fallback: importing works without a GPU (symbols can be inspected),
calling a compute entry without a gfx950 device returns a TK_ERROR_GPU_* code, and a missing
.so raises immediately.
"""
from ._lib import lib, TkError, check, LIB_PATH  # noqa: F401
from .llm import llm_step_probe, LlmStepProbe, STEP_EMBED, STEP_RMSNORM, STEP_RESIDUAL_FOLD, STEP_SWIGLU, STEP_QUANT, STEP_ROPE_APPEND, STEP_PV_JOIN, STEP_ATT_TILES, STEP_FUSED_NORM, STEP_FUSED_SWIGLU, STEP_WIDE_SWIGLU, ROUND_NONE, ROUND_F16, ROUND_BF16  # noqa: F401
from .llm import LlmHParams, LlmModel, LlmSession, LlmPipe, PipeHandle, ModelLoader, LlmRunner, MISTRAL_7B, TINY, attention_plan, lora_probe, gemv_probe, repack_probe, prefix_match, quantize_blocks, convert_bf16, matmul_float_probe, kv_shift_probe, kv_shift_probe_into, lookup_draft, lookup_accept, attention_plan_verify, attention_resident_limit, KV_F16, KV_Q8_0, kv_q8_probe_into, kv_q8_quantize_probe, kv_q8_attention_probe  # noqa: F401
from .llm import TokenLogprob, TOKEN_LOGPROB_DTYPE, LOGPROB_MAX_TOP, token_logprobs_probe, time_token_logprobs  # noqa: F401
from .llm import grammar_mask_probe, time_grammar_mask  # noqa: F401
from .llm import TYPE_F32, TYPE_F16, TYPE_Q4_0, TYPE_Q5_0, TYPE_Q8_0, TYPE_Q2_K, TYPE_Q3_K, TYPE_Q4_K, TYPE_Q5_K, TYPE_Q6_K, TYPE_IQ4_NL, TYPE_IQ4_XS, TYPE_Q4_1, TYPE_Q5_1, TYPE_BF16, TYPE_TQ1_0, TYPE_TQ2_0, FTYPE_TQ1_0, FTYPE_TQ2_0, FTYPE_Q4_1, FTYPE_Q5_1, FTYPE_IQ4_NL, FTYPE_IQ4_XS, FTYPE_Q4_0, FTYPE_Q5_0, FTYPE_Q8_0, FTYPE_Q2_K, FTYPE_Q2_K_S, FTYPE_Q3_K_S, FTYPE_Q3_K_M, FTYPE_Q4_K_S, FTYPE_Q4_K_M, FTYPE_Q5_K_S, FTYPE_Q5_K_M  # noqa: F401
from .vision import ObjectDetector, VisionPipeline, classify_attributes, preprocess, COCO80  # noqa: F401,E402
from .vision import DepthEstimator, depth_onnx_probe, fuse_data, fusion_reset, fusion_raw_distance  # noqa: F401,E402
from .vision import onnx_run, detector_post_probe, DetectorPostProbe, BOX_DTYPE, YOLO_MAX_CAND, YOLO_MAX_DET  # noqa: F401,E402
from .nn import GemmProbe, gemm_probe, gemm_code, attention_h3_probe, GEMM_F32, GEMM_F32_TALL, GEMM_F32_BIG, GEMM_H3_TALL, GEMM_H3_BIG  # noqa: F401,E402
from .nn import EdgeProbe, edge_probe, EDGE_FRAMES, EDGE_POWER, EDGE_LOGMEL_FINISH, EDGE_VAD_HEAD, EDGE_PREPROCESS, EDGE_DEPTH_MINMAX, EDGE_DEPTH_METRIC, EDGE_POSTPROCESS_DEPTH, EDGE_DEPTH_TO_POINTS, EDGE_BOX_ATTRIBUTES, PREPROCESS_CANONICAL, PREPROCESS_SCALED  # noqa: F401,E402
from .nn import NnRowProbe, nn_row_probe, ROW_CONV_STEM, ROW_IM2COL, ROW_IM2COL1D, ROW_MAXPOOL5, ROW_UPSAMPLE2X, ROW_COPY_COLS, ROW_LAYERNORM, ROW_SOFTMAX_ROWS, ROW_ADD_ROWS, ROW_EMBED_ROWS, ROW_ATTEND1  # noqa: F401,E402
from .nn import SOFTMAX_GENERIC, SOFTMAX_REG, SOFTMAX_WAVE, IM2COL_ELEMENT, IM2COL_V4  # noqa: F401,E402
from .pick import LogitAdjust, logit_adjust_rows, logit_adjust_probe, logit_adjust_probe_into, lang_pick_probe  # noqa: F401,E402
from .pick import TokenPickProbe, token_pick_probe, sampling_rows, SAMPLING_DTYPE, PICK_ARGMAX, PICK_ARGMAX_ROWS, PICK_ROWS, PICK_ROWS_FILTERED  # noqa: F401,E402
from .audio import Asr, Vad, WhisperHP, WHISPER_TINY_EN, AudioPipeline, whisper_lang_code, whisper_lang_id  # noqa: F401,E402
from .cortex import Cortex, RocmDispatcher, PreprocessParams, DepthPostParams, DepthToPointsParams, Float3  # noqa: F401,E402
