/*
 * tk_box_attr.h — the per-pixel arithmetic of the per-box attribute classifiers (reference: src/vision/tk_attribute_classifier.c), shared by
 * k_box_attributes (csrc/vision/tk_vision_engine.hip) and the CPU oracle, so that both evaluate the same float / double operations:
 *   r,g,b = u8 / 255.0f;  v = max, delta = max - min, s = delta / max  (s = 0 when max = 0)
 *   h = 60 * ((g - b) / delta | 2 + (b - r) / delta | 4 + (r - g) / delta), + 360 when negative   (the constants are doubles in the
 *   reference: a float op double op rounds once more on the store to float, reproduced with explicit double arithmetic)
 *   s < 0.1 (double compare): black (v < 0.1) / white (v > 0.9) / gray, else six 60-degree hue bins starting at 330.
 * Luminance is the integer 299 / 587 / 114 per mille; a door is closed when edges / (w * h) > 0.1 (float quotient, double compare).
 */
#ifndef TK_BOX_ATTR_H
#define TK_BOX_ATTR_H

#include "tk_exact_math.h"

/* colour bin 0..8 of one pixel: red, yellow, green, cyan, blue, magenta, black, white, gray; -1: NaN hue, counted in no bin */
TK_HD int tk_color_bin(uint8_t R, uint8_t G, uint8_t B) {
    const float r = tk_divf((float)R, 255.0f), g = tk_divf((float)G, 255.0f), b = tk_divf((float)B, 255.0f);
    const float gb_max = g > b ? g : b, gb_min = g < b ? g : b;
    const float mx = r > gb_max ? r : gb_max, mn = r < gb_min ? r : gb_min;
    const float delta = mx - mn, v = mx;
    float s = 0.0f, h = 0.0f;
    if ((double)mx > 0.0) {
        s = tk_divf(delta, mx);
        if (r >= mx) h = tk_divf(g - b, delta);
        else if (g >= mx) h = (float)(2.0 + (double)tk_divf(b - r, delta));
        else h = (float)(4.0 + (double)tk_divf(r - g, delta));
        h = (float)((double)h * 60.0);
        if ((double)h < 0.0) h = (float)((double)h + 360.0);
    }
    if ((double)s < 0.1) return (double)v < 0.1 ? 6 : ((double)v > 0.9 ? 7 : 8);
    if (h < 30.0f || h >= 330.0f) return 0;
    if (h < 90.0f) return 1;
    if (h < 150.0f) return 2;
    if (h < 210.0f) return 3;
    if (h < 270.0f) return 4;
    if (h < 330.0f) return 5;
    return -1;
}

TK_HD int tk_luma(const uint8_t* p) { return (int)(uint8_t)((p[0] * 299 + p[1] * 587 + p[2] * 114) / 1000); }

/* strong vertical edge between the rows above and below a pixel */
TK_HD int tk_edge_between(const uint8_t* above, const uint8_t* below) {
    const int d = tk_luma(above) - tk_luma(below);
    return (d < 0 ? -d : d) > 100;
}

/* the density test.  The area is formed in 64 bits: the reference multiplies in `int` (:137), which is the same number for every box whose
 * area is below 2^31 and undefined above; here a larger box has its true area, so its density cannot come out of a wrapped product. */
TK_HD int tk_door_closed(int edges, int bw, int bh) {
    const float density = tk_divf((float)edges, (float)((int64_t)bw * bh));
    return (double)density > 0.1 ? 1 : 0;
}

#endif
