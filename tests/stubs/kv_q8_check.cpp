/*
 * kv_q8_check — csrc/common/tk_kv_q8.h in a stand-alone host program (tests/test_kv_q8_cpu.py builds it with -fsanitize=address,undefined and reads
 * its output).
 *   kv_q8_check round            tk_kv_q8_roundf on the edge values, as "bits_in bits_out" lines — among them nextafter(0.5, 0), which no f16 row
 *                                reaches through the cache (x * id with f16 x never lands on it) and which truncf(v + 0.5f) gets wrong
 *   kv_q8_check rows FILE HD     FILE holds n rows of HD f16 values; prints per row the int8 values and the scale bits of tk_kv_q8_row, then runs
 *                                tk_kv_q8_attention_row over the rows as one (sequence, KV head) run for 1, 2 and 4 query heads and prints the
 *                                output bits
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "tk_kv_q8.h"

int main(int argc, char** argv) {
    if (argc >= 2 && strcmp(argv[1], "round") == 0) {
        const float edge[] = {0.5f, -0.5f, nextafterf(0.5f, 0.0f), -nextafterf(0.5f, 0.0f), 1.5f, -1.5f, 2.5f, -2.5f, 126.5f, -126.5f, 127.0f, -127.0f, 0.0f, -0.0f,
                              0.25f, 126.49999f, 1.4999999f, 127.00001f};
        for (float v : edge) printf("%08x %08x\n", tk_f32_bits(v), tk_f32_bits(tk_kv_q8_roundf(v)));
        return 0;
    }
    if (argc >= 4 && strcmp(argv[1], "rows") == 0) {
        const int hd = atoi(argv[3]);
        if (hd < 32 || hd % 32) return 2;
        FILE* f = fopen(argv[2], "rb");
        if (!f) return 2;
        std::vector<uint16_t> rows;
        uint16_t buf[256];
        size_t n;
        while ((n = fread(buf, 2, 256, f)) > 0) rows.insert(rows.end(), buf, buf + n);
        fclose(f);
        const int T = (int)(rows.size() / (size_t)hd), nb = hd / TK_KV_Q8_BLOCK;
        if (T < 1 || rows.size() != (size_t)T * hd) return 2;
        std::vector<int8_t> q((size_t)T * hd);
        std::vector<uint16_t> d((size_t)T * nb);
        for (int t = 0; t < T; ++t) {
            tk_kv_q8_row(rows.data() + (size_t)t * hd, hd, q.data() + (size_t)t * hd, d.data() + (size_t)t * nb);
            printf("row");
            for (int i = 0; i < hd; ++i) printf(" %d", (int)q[(size_t)t * hd + i]);
            printf(" |");
            for (int b = 0; b < nb; ++b) printf(" %u", (unsigned)d[(size_t)t * nb + b]);
            printf("\n");
        }
        for (int gq = 1; gq <= 4; gq *= 2) { /* keys = values = the rows; queries = the first rows' dequantised values */
            std::vector<float> qv((size_t)gq * hd), scratch((size_t)T * gq), out((size_t)gq * hd);
            for (int h = 0; h < gq; ++h)
                for (int i = 0; i < hd; ++i) qv[(size_t)h * hd + i] = tk_kv_q8_value(d[(size_t)(h % T) * nb + i / TK_KV_Q8_BLOCK], q[(size_t)(h % T) * hd + i]);
            tk_kv_q8_attention_row(qv.data(), gq, hd, T, q.data(), d.data(), q.data(), d.data(), scratch.data(), out.data());
            printf("att %d", gq);
            for (float v : out) printf(" %08x", tk_f32_bits(v));
            printf("\n");
        }
        return 0;
    }
    fprintf(stderr, "usage: kv_q8_check round | rows FILE HEAD_DIM\n");
    return 2;
}
