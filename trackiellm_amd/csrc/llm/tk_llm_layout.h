/*
 * tk_llm_layout.h — HBM layouts of the MI355X LLM path.
 *
 * GGUF k-quant blocks are kept bit-for-bit (the same quantised values, and the file's bytes per 256 weights
 * for every type of tk_type_desc_of but Q3_K, whose scales are stored unpacked; Q8_0 / Q4_0 / Q5_0 / IQ4_NL / Q4_1 / Q5_1: eight 34- / 18- / 22- / 18- / 20- / 24-byte blocks per 256 weights; IQ4_XS: its scales unpacked too; TQ1_0: its base-3 digits as 2-bit codes, 66 for 54 bytes) but re-tiled at load time so that one wavefront's 16-byte-per-lane
 * load is a contiguous 1 KiB run that already IS an MFMA operand:
 *
 *  Weight tile = 16 weight rows x 256 k (one super-block column).  Lane l = (n = l & 15, g = l >> 4)
 *  owns weight row n and the 8-wide k-slice g of every 32-wide sub-block, i.e. exactly the
 *  B-operand fragment of v_mfma_i32_16x16x32_i8  (B[k = 8g + t][j = n]).
 *
 *  Q4_K tile (2304 B = 16 x 144):
 *      [0    ,1024)  load 0: lane l -> 4 dwords, dword s = sub-block s      (k = 32 s + 8 g + 0..7)
 *      [1024 ,2048)  load 1: lane l -> 4 dwords, dword s = sub-block 4 + s
 *                    dword byte t = q[k0 + t] | q[k0 + 4 + t] << 4   (k0 = 32 j + 8 g)
 *      [2048 ,2304)  16 rows x {f16 d, f16 dmin, 12 B packed 6-bit scales/mins} verbatim
 *  Q5_K tile (2816 B = 16 x 176):
 *      [0    ,2048)  the low nibbles as the two loads of the Q4_K tile
 *      [2048 ,2560)  lane l -> 2 dwords: the high bits of the 64 weights whose nibbles lane l holds; dword i covers sub-blocks
 *                    4 i + s (s = 0..3): the high bit of the weight in byte y of operand dword lo / hi (k0 + y / k0 + 4 + y) of
 *                    sub-block 4 i + s sits at bit 8y + s / 8y + 4 + s, so one shift and one mask put it at bit 4 of its byte
 *      [2560 ,2816)  16 rows x {f16 d, f16 dmin, 12 B packed 6-bit scales/mins} verbatim
 *  Q2_K tile (1344 B = 16 x 84): operand dword o = 2 j + hh of lane l as in the Q3_K tile below
 *      [0    ,1024)  one load: lane l -> 4 dwords; bits 8 t + 2 (o & 3) .. + 1 of dword o >> 2 = q of weight t of operand dword o
 *                    (one shift and one mask give the four byte selectors 0..3 of an operand dword)
 *      [1024 ,1280)  16 rows x 16 (scale, min) bytes as the block holds them (low nibble scale, high nibble min), byte 8 h + j = group
 *                    2 j + h: a lane reads the 8 bytes of its k half
 *      [1280 ,1344)  16 x {f16 d, f16 dmin}
 *  Q8_0 tile (4352 B = 16 x 272 = 16 rows x eight 34-byte blocks): a 256-k run of 16 rows, the int8 quants as the file holds them
 *      [0    ,4096)  four loads: load i, lane l -> 4 dwords, dword 2 e + hh = the weights k0 + 4 hh .. + 3 (k0 = 32 (2 i + e) + 8 g) of
 *                    32-block 2 i + e: the lane's eight weights of each block, already the B operand bytes (dwords 2 e, 2 e + 1 of
 *                    load i are one v_mfma_i32_16x16x32_i8 operand; the whole load is the 16x16x64 operand of the other tiles)
 *      [4096 ,4352)  16 rows x 8 f16 d, row n's eight block scales in block order: one 16-byte read per lane
 *  Q4_0 tile (2304 B = 16 x 144 = 16 rows x eight 18-byte blocks): a 256-k run of 16 rows, the stored nibbles q (0..15, w = d (q - 8))
 *      [0    ,2048)  the two loads of the Q4_K tile with 32-block 4 L + s in place of sub-block 4 L + s: dword s of load L, byte t =
 *                    q[k0 + t] | q[k0 + 4 + t] << 4 (k0 = 8 g, weights counted inside the block)
 *      [2048 ,2304)  16 rows x 8 f16 d in block order, as the Q8_0 tile's tail
 *  Q5_0 tile (2816 B = 16 x 176 = 16 rows x eight 22-byte blocks): the stored q (0..31, w = d (q - 16))
 *      [0    ,2048)  the low nibbles as the two loads of the Q4_0 tile
 *      [2048 ,2560)  lane l -> 2 dwords, the high bits as the Q5_K tile arranges them: dword L covers blocks 4 L + s, the bit of the
 *                    weight in byte y of operand dword lo / hi (k0 + y / k0 + 4 + y) of block 4 L + s at bit 8y + s / 8y + 4 + s
 *      [2560 ,2816)  16 rows x 8 f16 d in block order
 *  The kernels turn a masked nibble dword (plus the high bits at bit 4) into int8 q - 8 / q - 16 with one add and one xor,
 *  (x + 0x78787878) ^ 0x80808080 / (x + 0x70707070) ^ 0x80808080: no byte carries (0x78 + 15 and 0x70 + 31 stay below 0x100), and the
 *  result is the B operand the Q8_0 chains take.
 *  Q4_1 tile (2560 B = 16 x 160 = 16 rows x eight 20-byte blocks): the stored q (0..15, w = d q + m), unsigned as it goes into the int8 operand
 *      [0    ,2048)  the two nibble loads of the Q4_0 tile
 *      [2048 ,2560)  16 rows x 32 B: row n's eight f16 d in block order, then its eight f16 m: two 16-byte reads per lane
 *  Q5_1 tile (3072 B = 16 x 192 = 16 rows x eight 24-byte blocks): the stored q (0..31, w = d q + m)
 *      [0    ,2560)  the nibble loads and the high bits of the Q5_0 tile
 *      [2560 ,3072)  16 rows x 32 B: eight d, then eight m, as the Q4_1 tile's tail
 *  Neither needs an offset: the nibble dword (plus the high bits at bit 4) IS the B operand.  The min term m_j * sum_k a_k takes the
 *  block's activation sum from the matrix pipe (the A operand against an all-ones B), in the accumulator layout of P_j.
 *  IQ4_NL tile (2304 B): the Q4_0 tile byte for byte (same repack kernel, fragment and load); the nibble is a code-book index
 *  IQ4_XS tile (2304 B = 16 x 144; the block has 136 B): a 256-weight block of 16 rows
 *      [0    ,2048)  the two nibble loads of the Q4_0 tile with sub-block j in place of 32-block j
 *      [2048 ,2304)  16 rows x 16 B: the eight sub-block scales s_j = ls_j - 32 as int8 (bytes 0..7), the f16 d (bytes 8, 9), six zero
 *                    bytes: one 16-byte read per lane where the Q4_0 tile has its eight d, so the fragment and load are the Q4_0 tile's
 *                    too.  A tighter tail (the block's own 8 bytes: d, scales_h, scales_l = 2176 B) was not taken: it would need a load
 *                    and a 6-bit unpack of its own in all three families for 5.6 % of the tile's bytes
 *  The kernels turn four nibbles of a dword into int8 kv[q] with three v_perm_b32: the code book is four constant dwords, two permutes
 *  on q & 7 look up both halves and a third picks per byte by bit 3.  The result is the B operand the Q8_0 chains take; the block scale
 *  is d (IQ4_NL) or d * (float)s_j in fp32 (IQ4_XS, exact).
 *  Q3_K tile (1824 B = 16 x 114): weights stored as u = q + 4 (0..7).  Operand dword o = 2 j + hh (o = 0..15) of lane l holds the four
 *  weights k0 + 4 hh + t (t = 0..3, k0 = 32 j + 8 g) of sub-block j, as in the tiles above
 *      [0    ,1024)  one load: lane l -> 4 dwords; bits 8 t + 2 (o & 3) .. + 1 of dword o >> 2 = u & 3 of weight t of operand dword o
 *      [1024 ,1536)  lane l -> 2 dwords; bit 8 t + (o & 7) of dword o >> 3 = u >> 2 of weight t of operand dword o
 *                    (one shift and one mask per part put the four 3-bit u of an operand dword at bits 0..2 of its bytes)
 *      [1536 ,1792)  16 rows x 16 int8 group scales s = sc6 - 32, byte 8 h + j = group 2 j + h: a lane reads the 8 bytes of its k half
 *      [1792 ,1824)  16 x f16 d
 *  TQ2_0 tile (1056 B = 16 x 66): the 2-bit codes c (0..3, w = (c - 1) d), operand dword o = 2 j + hh of lane l as in the Q3_K tile above
 *      [0    ,1024)  one load, the Q2_K tile's: lane l -> 4 dwords; bits 8 t + 2 (o & 3) .. + 1 of dword o >> 2 = c of weight t of operand
 *                    dword o (one shift and one mask give the four byte selectors 0..3 of an operand dword)
 *      [1024 ,1056)  16 x f16 d
 *  The kernels turn the selectors into int8 c - 1 with one v_perm_b32 on the constant bytes {-1, 0, 1, 2}: code 3 gives +2, no byte carries.
 *  TQ1_0 tile: the TQ2_0 tile.  The repack (TkBlock<TK_TYPE_TQ1_0>::code, tk_ggml_blocks.h) decodes the block's base-3 bytes once, at load, and writes the trits t (0..2) as codes, so
 *  a TQ1_0 matrix streams 66 bytes per 256 weights where its file holds 54, and runs the kernels a TQ2_0 matrix runs
 *  Q6_K tile (3360 B = 16 x 210): weights stored as 6-bit two's complement q' = (q - 32) & 63
 *      [0    ,2048)  two loads as above holding the LOW nibbles of q'
 *      [2048 ,3072)  lane l -> 4 dwords; dword u covers sub-blocks 2u, 2u+1: the 2 high bits of
 *                    the 4 weights that land in byte y of operand dword T_t sit at bits 8y+2t, 8y+2t+1
 *                    (T_0/T_1 = lo/hi dword of sub-block 2u, T_2/T_3 = lo/hi dword of 2u+1)
 *      [3072 ,3328)  16 rows x 16 int8 group scales verbatim
 *      [3328 ,3360)  16 rows x f16 d
 *  The kernel rebuilds int8 = q' << 2 = 4 (q - 32) with two shift/mask ops per dword and folds
 *  the factor 4 into the block scale (exact: power of two).
 *
 *  Tiles of one 16-row group are contiguous over k:  tiles[row_tile][block].
 *
 *  Activations (Q8_K-style, the reference CPU engine's numerics — oracle/tk_oracle_llm.cpp):
 *      aq  : int8   [K/64][4 g][16 row slot][2 sub-blocks][8]   == the A-operand image of v_mfma_i32_16x16x64_i8: lane
 *                    (slot, g) reads its 16 bytes (k-slice g of two consecutive 32-wide sub-blocks) with ONE ds_read_b128
 *                    (1.6x the LDS bandwidth of two 8-byte reads on gfx950, tools/lds_rate.hip); a K-range is one
 *                    contiguous run that is DMA'd into LDS
 *      ad  : float  [K/256][16]        block scale amax/127
 *      abs : int8   [K/256][2][16][8]  per-sub-block sums of the int8 values (the Q4_K "min" term) split as
 *                                      sum = 64 h + l: image 0 holds l (0..63), image 1 holds h, byte j = sub-block j —
 *                                      the A operand of the MFMA that contracts them with the 6-bit mins
 *      abs16: f16   [K/256][2][16][8]  the same sums as sum = 2 hh + ll (|hh| <= 2032, ll in {0, 1}: exact in f16) — the batched kernel
 *                                      contracts them with (2 m_j, m_j) in ONE v_mfma_f32_16x16x32_f16 (exact: every partial sum < 2^24)
 *  "row slot" b < 16 is a (sequence, position) row of the current pass; a pass holds up to TK_MAX_TILES such
 *  16-row M-tiles (row r lives in tile r / 16, slot r % 16), each with its own aq / ad / abs image.
 */
#ifndef TK_LLM_LAYOUT_H
#define TK_LLM_LAYOUT_H

#include <stdint.h>

#define TK_TILE_ROWS 16
/* the tile sizes documented above; tk_type_desc_of (common/tk_ggml_blocks.h) takes them as each type's tile_bytes and checks them */
#define TK_Q2K_TILE_BYTES 1344
#define TK_Q3K_TILE_BYTES 1824
#define TK_Q4K_TILE_BYTES 2304
#define TK_Q5K_TILE_BYTES 2816
#define TK_Q6K_TILE_BYTES 3360
#define TK_Q8_0_TILE_BYTES 4352
#define TK_Q4_0_TILE_BYTES 2304
#define TK_Q5_0_TILE_BYTES 2816
#define TK_IQ4_NL_TILE_BYTES TK_Q4_0_TILE_BYTES
#define TK_IQ4_XS_TILE_BYTES 2304
#define TK_Q4_1_TILE_BYTES 2560
#define TK_Q5_1_TILE_BYTES 3072
#define TK_TQ2_0_TILE_BYTES 1056 /* TQ1_0's too: it is installed as this tile */
#define TK_ROW_SLOTS 16  /* rows of one MFMA M-tile */
#define TK_MAX_TILES 16   /* M-tiles per pass: a weight tile is unpacked once and multiplied against all of them */
#define TK_MAX_ROWS (TK_ROW_SLOTS * TK_MAX_TILES)

/* per M-tile sizes; tile m of a buffer starts at m * (these) */
#define TK_AQ_BYTES(K) ((size_t)(K) * TK_ROW_SLOTS)
#define TK_AD_FLOATS(K) ((size_t)(K) / 256 * TK_ROW_SLOTS)
#define TK_ABS_BYTES(K) ((size_t)(K) / 256 * 256)

#endif
