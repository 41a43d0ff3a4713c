// fmt_out.h — the bounded output buffer of the host formatters (tsv_format.cpp, json_format.cpp): bytes into a buffer of
// `cap`, counted beyond it (the convention of kaamer_format_positions: need = f(NULL, 0)).
#pragma once
#include <stdint.h>
#include <string.h>

struct Out {
    char *buf;
    uint64_t cap, len = 0;
    Out(char *b, uint64_t c) : buf(b), cap(b ? c : 0) {}
    void put(char c) { if (len < cap) buf[len] = c; len++; }
    void put(const char *s, uint64_t n)
    {
        if (n && len < cap) memcpy(buf + len, s, (size_t)(n < cap - len ? n : cap - len));
        len += n;
    }
    void lit(const char *s) { put(s, strlen(s)); }
    void put_u64(uint64_t v)
    {
        char tmp[24];
        int n = 0;
        do { tmp[n++] = (char)('0' + v % 10); v /= 10; } while (v);
        while (n) put(tmp[--n]);
    }
    void put_int(int64_t v)   // strconv.Itoa
    {
        if (v < 0) { put('-'); put_u64((uint64_t)0 - (uint64_t)v); }
        else put_u64((uint64_t)v);
    }
    void finish() { if (cap) buf[len < cap ? len : cap - 1] = '\0'; }
};
