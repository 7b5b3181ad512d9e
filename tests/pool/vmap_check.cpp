/*
 * Memory check of the verbose-mapping reader (ntl_vmap_*, ntlink_amd/csrc/ntl_io.cpp): the reader is fed files that end where they
 * should not -- every prefix of a good file, lines without a newline at the end, empty tokens, empty fields, 11-digit numbers -- whole
 * and in blocks of a few bytes, on one parser thread and on several, and every block it accepts is copied out into arrays of exactly
 * the sizes it announced.  One line per failed check, exit status 1 on any.  Built with ntl_io.cpp by tests/test_vmap_check.py
 * (g++ -fsanitize=address,undefined) and run as a child process: no GPU, no Python.
 */
#include "../../include/ntlink_amd.h"

#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>
#include <string>
#include <vector>

static int g_failed = 0;
#define CHECK(cond, ...)                                                                   \
    do {                                                                                   \
        if (!(cond)) {                                                                     \
            g_failed++;                                                                    \
            printf("FAILED %s:%d %s: ", __func__, __LINE__, #cond);                        \
            printf(__VA_ARGS__);                                                           \
            printf("\n");                                                                  \
        }                                                                                  \
    } while (0)

static const char CTG_NAMES[] = "c1ctg2";
static const uint64_t CTG_OFF[] = {0, 2, 6};

struct Totals { uint64_t reads = 0, maps = 0, hits = 0; int rc = 0; std::string err; };

/* reads `text` through a file in blocks of max_bytes; the arrays are heap blocks of exactly the announced sizes */
static Totals read_all(const std::string &dir, const std::string &text, uint64_t max_bytes)
{
    Totals t;
    const std::string path = dir + "/in.tsv";
    FILE *f = fopen(path.c_str(), "wb");
    if (!f) { t.rc = -100; return t; }
    fwrite(text.data(), 1, text.size(), f);
    fclose(f);
    ntl_vmap *r = nullptr;
    if ((t.rc = ntl_vmap_open(path.c_str(), CTG_NAMES, CTG_OFF, 2, &r))) return t;
    for (;;) {
        uint64_t n = 0;
        if ((t.rc = ntl_vmap_next(r, max_bytes, &n))) { t.err = ntl_vmap_error(r); break; }
        if (!n) break;
        uint64_t n2 = 0, nm = 0, nh = 0, nb = 0;
        ntl_vmap_sizes(r, &n2, &nm, &nh, &nb);
        CHECK(n2 == n && nm >= n && nh >= nm, "sizes %llu %llu %llu", (unsigned long long)n2, (unsigned long long)nm, (unsigned long long)nh);
        std::vector<char> names(nb);
        std::vector<uint64_t> name_off(n + 1);
        std::vector<uint32_t> map_off(n + 1), anchors(nm);
        std::vector<ntl_mapping> maps(nm);
        std::vector<ntl_hit> hits(nh);
        const int rc = ntl_vmap_copy(r, names.data(), name_off.data(), map_off.data(), maps.data(), anchors.data(), hits.data());
        CHECK(rc == 0, "copy %d", rc);
        CHECK(name_off[n] == nb && map_off[0] == 0 && map_off[n] == nm, "offsets");
        uint64_t h = 0;
        for (uint64_t m = 0; m < nm; m++) {
            CHECK(maps[m].hit_off == h && maps[m].n_hits >= 1 && maps[m].read < n, "mapping %llu", (unsigned long long)m);
            CHECK(map_off[maps[m].read] <= m && m < map_off[maps[m].read + 1], "mapping %llu in its read's range", (unsigned long long)m);
            CHECK(maps[m].ctg == 0xFFFFFFFFu || maps[m].ctg < 2, "contig %u", maps[m].ctg);
            h += maps[m].n_hits;
        }
        CHECK(h == nh, "hits %llu of %llu", (unsigned long long)h, (unsigned long long)nh);
        t.reads += n; t.maps += nm; t.hits += nh;
    }
    ntl_vmap_close(r);
    return t;
}

int main()
{
    char tmpl[] = "/tmp/vmap_check_XXXXXX";
    const char *d = mkdtemp(tmpl);
    if (!d) { printf("FAILED mkdtemp\n"); return 1; }
    const std::string dir = d;
    std::string good;
    for (int r = 0; r < 12; r++)
        for (int m = 0; m <= r % 3; m++) {
            good += "read" + std::to_string(r) + "\t" + (m == 0 ? "c1" : m == 1 ? "ctg2" : "elsewhere") + "\t" + std::to_string(7 + m) + "\t";
            for (int h = 0; h <= (r * 5 + m) % 9; h++)
                good += std::string(h ? " " : "") + std::to_string(100 * h + r) + (h & 1 ? ":+_" : ":-_") + std::to_string(4000000000u + (unsigned)h) + ":+";
            good += "\n";
        }
    const char *const chunk_env[] = {nullptr, "16"};
    for (const char *chunk : chunk_env) { /* one parser thread; ranges of a line or two on the worker pool */
        if (chunk) setenv("NTL_IO_MIN_CHUNK", chunk, 1);
        const uint64_t sizes[] = {0, 1, 7, 64, 300};
        const Totals whole = read_all(dir, good, 0);
        CHECK(whole.rc == 0 && whole.reads == 12 && whole.maps == 24, "the good file: rc %d, %llu reads, %llu lines (%s)", whole.rc,
              (unsigned long long)whole.reads, (unsigned long long)whole.maps, whole.err.c_str());
        for (uint64_t mb : sizes) {
            /* a line without a newline at the end is a line */
            const Totals a = read_all(dir, good.substr(0, good.size() - 1), mb);
            CHECK(a.rc == 0 && a.reads == whole.reads && a.maps == whole.maps && a.hits == whole.hits, "no newline at the end, blocks of %llu: rc %d (%s)",
                  (unsigned long long)mb, a.rc, a.err.c_str());
            /* truncated files: every prefix parses or is refused with a line number, and nothing is read or written out of bounds */
            for (size_t cut = 0; cut < good.size(); cut += (mb == 0 || mb == 7 ? 1 : 13)) {
                const Totals p = read_all(dir, good.substr(0, cut), mb);
                CHECK(p.rc == 0 || (p.rc == NTL_EINVAL && p.err.compare(0, 5, "line ") == 0), "prefix of %zu bytes, blocks of %llu: rc %d (%s)", cut,
                      (unsigned long long)mb, p.rc, p.err.c_str());
                CHECK(p.maps <= whole.maps && p.hits <= whole.hits, "prefix of %zu bytes", cut);
            }
        }
        struct { const char *text; const char *line; } bad[] = {
            {"r\tc1\t1\t1:+_2:+  3:+_4:+\n", "line 1:"},                          /* an empty token */
            {"r\tc1\t1\t 1:+_2:+\n", "line 1:"},
            {"r\tc1\t1\t1:+_2:+\nr\tc1\t1\t\t\n", "line 2:"},                      /* empty fields */
            {"r\tc1\t1\t1:+_2:+\n\t\t\t\n", "line 2:"},
            {"r\tc1\t1\t1:+_2:+\nr\tc1\t\t1:+_2:+\n", "line 2:"},
            {"r\tc1\t1\t12345678901:+_2:+\n", "line 1:"},                          /* 11-digit numbers */
            {"r\tc1\t1\t1:+_2:+\nq\tc1\t1\t1:+_12345678901:+\n", "line 2:"},
            {"r\tc1\t12345678901\t1:+_2:+\n", "line 1:"},
            {"r\tc1\t1\t1:+_99999999999999999999999999999999999999:+\n", "line 1:"},
            {"r\tc1\t1\t1:+_2:+\nq\tc1\t1\t1:+_2:\n", "line 2:"},
            {"r\tc1\t1\t1:+_2:+\nq\tc1\t1\t1:+_", "line 2:"},
            {"r\tc1\t1\t1:+_2:+\nq\tc1\t1\t1", "line 2:"},
            {"r\tc1\t1\t1:+_2:+\nq\tc1\t1", "line 2:"},
            {"\n", "line 1:"},
        };
        for (auto &b : bad)
            for (uint64_t mb : {(uint64_t)0, (uint64_t)5}) {
                const Totals t = read_all(dir, b.text, mb);
                CHECK(t.rc == NTL_EINVAL && t.err.compare(0, strlen(b.line), b.line) == 0, "%s blocks of %llu: rc %d (%s)", b.line, (unsigned long long)mb,
                      t.rc, t.err.c_str());
            }
    }
    unlink((dir + "/in.tsv").c_str());
    rmdir(dir.c_str());
    if (g_failed) { printf("vmap_check: %d checks failed\n", g_failed); return 1; }
    printf("vmap_check: ok\n");
    return 0;
}
