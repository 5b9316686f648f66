// Memory-safety check of the JPEG encoder's host half (csrc/fs_jpegenc.hip), stand-alone and host only: fs_jpeg_encode_plan / fs_jpeg_write on synthetic
// coefficient buffers in exact-size heap blocks, with caps from 0 to the exact file size, under AddressSanitizer + UBSan.  From the repository root:
//   clang++ -x c++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -I tests/emu -I faststyle_amd/csrc
//           tools/jpeg_write_check.cpp faststyle_amd/csrc/fs_jpegenc.hip -o /tmp/jpeg_write_check -lpthread && /tmp/jpeg_write_check
// (the kernels of that file compile against the emulator header and are not run here).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cstdarg>
#include <vector>
#include "../include/faststyle_io.h"
namespace fs { int set_error(int code, const char*, ...) { return code; } int knob(int) { return 0; } }
int main() {
    unsigned seed = 1;
    auto rnd = [&]() { seed = seed * 1664525u + 1013904223u; return seed >> 8; };
    int files = 0, refused = 0;
    const int geo[][5] = {{1,1,3,2,2},{17,9,3,2,2},{37,53,3,2,1},{64,48,3,1,1},{33,31,1,1,1},{8,8,3,2,2}};
    for (auto& g : geo) for (int amp : {0, 3, 60, 1023}) for (int rep = 0; rep < 6; ++rep) {
        fs_jpeg_info info;
        if (fs_jpeg_encode_plan(g[0], g[1], g[2], g[3], g[4], &info)) return 1;
        // exact-size heap blocks: any access outside them is reported
        int16_t* coef = (int16_t*)malloc(info.coef_bytes);
        for (size_t i = 0; i < info.coef_count; ++i) coef[i] = amp ? (int16_t)((int)(rnd() % (2 * amp + 1)) - amp) : 0;
        if (rep == 5) for (size_t i = 0; i < info.coef_count; ++i) coef[i] = (i & 63) ? (int16_t)(rnd() & 1 ? -1 : 255) : (int16_t)(rnd() % 2047 - 1023);  // many 0xFF bytes
        for (size_t b = 0; b < info.coef_count / 64; ++b) coef[b * 64] = (int16_t)((int)(rnd() % 2001) - 1000);
        uint16_t* qt = (uint16_t*)((char*)coef + info.qt_offset);
        for (int i = 0; i < 192; ++i) qt[i] = i < 64 * (g[2] == 3 ? 3 : 1) ? 1 + rnd() % 255 : 0;
        size_t bound = fs_jpeg_write_bound(&info), n = 0;
        unsigned char* big = (unsigned char*)malloc(bound);
        int rc = fs_jpeg_write(&info, coef, info.coef_bytes, big, bound, &n);
        if (rc != 0 || n > bound || n < 4 || big[n - 2] != 0xFF || big[n - 1] != 0xD9) { printf("bad write rc %d n %zu bound %zu\n", rc, n, bound); return 1; }
        ++files;
        for (size_t cap : {(size_t)0, (size_t)1, (size_t)19, n / 3, n / 2, n - 2, n - 1, n}) {
            unsigned char* out = (unsigned char*)malloc(cap ? cap : 1);
            size_t m = 0;
            rc = fs_jpeg_write(&info, coef, info.coef_bytes, cap ? out : out, cap, &m);
            if (cap < n ? rc != -3 : (rc != 0 || m != n || memcmp(out, big, n))) { printf("cap %zu of %zu: rc %d\n", cap, n, rc); return 1; }
            refused += rc == -3;
            free(out);
        }
        free(big);
        free(coef);
    }
    printf("ok: %d files, %d tight caps refused\n", files, refused);
    return 0;
}
