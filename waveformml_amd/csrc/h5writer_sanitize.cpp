// h5writer_sanitize.cpp -- standalone driver of libwfh5w's C ABI (include/wfh5w.h) for the sanitizer build:
//   make -C waveformml_amd/csrc asan_writer  -> ../lib/h5writer_sanitize_asan  (h5writer.cpp + this file, -fsanitize=address,undefined)
//   ../lib/h5writer_sanitize_asan <scratch dir>
// No Python in the sanitized process (as h5_sanitize.cpp).  The driver
//   1. writes a file through every output entry point (a Chanmap table, a record table from an explicit description in
//      several appends across the 1024-row chunk size, attributes), reads it back through every input entry point and
//      compares bytes, members and attributes; copies it (copy_dataset, create_table_like, copy_table_attrs, appends)
//      and compares again;
//   2. walks the input entry points -- and a copy through the output ones -- over DAMAGED copies: truncated at several
//      lengths, and with bytes flipped inside the tables' payload (the raw gzip chunks; flips in object headers are
//      libhdf5's to survive, and the image's 1.10.6 does not: see h5_sanitize.cpp), plus bad arguments on the intact
//      file.  A damaged file may be refused or read as garbage values; nothing may crash or trip a sanitizer.
// Exit code 0 = every call returned and the intact round trips compared equal.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <unistd.h>

#include <string>
#include <vector>

#include <hdf5.h>

#include "../../include/wfh5w.h"

static long g_calls = 0, g_ok = 0, g_failed = 0;

static int note(int rc) {
    ++g_calls;
    if (rc == WFH5W_OK) ++g_ok; else ++g_failed;
    return rc;
}

#define MUST(expr)                                                                                  \
    do {                                                                                            \
        if (note(expr) != WFH5W_OK) {                                                               \
            fprintf(stderr, "h5writer_sanitize: %s failed: %s\n", #expr, wfh5w_last_error());       \
            return 1;                                                                               \
        }                                                                                           \
    } while (0)

static wfh5w_member mk(const char *name, int64_t off, int kind, int count) {
    wfh5w_member m;
    memset(&m, 0, sizeof(m));
    snprintf(m.name, sizeof(m.name), "%s", name);
    m.offset = off;
    m.kind = kind;
    m.count = count;
    return m;
}

static const int64_t ITEM = 54;      // 2 mod 4, with a hole at [50, 54)
static const int64_t ROWS = 2500;    // three chunks of 1024

static std::vector<wfh5w_member> layout() {
    return {mk("evt", 0, WFH5W_I64, 1), mk("coord", 8, WFH5W_I32, 3), mk("waveform", 20, WFH5W_I16, 6),
            mk("EZ", 32, WFH5W_F32, 2), mk("t", 40, WFH5W_F64, 1), mk("tag", 48, WFH5W_I16, 1)};
}

static int write_file(const std::string &path, const std::vector<unsigned char> &rows) {
    wfh5w_out *o = nullptr;
    MUST(wfh5w_create(path.c_str(), &o));
    const wfh5w_member cm[] = {mk("chan", 0, WFH5W_I32, 1), mk("pos", 4, WFH5W_F32, 2)};
    MUST(wfh5w_create_table(o, "Chanmap", cm, 2, 12));
    std::vector<unsigned char> chan(12 * 20);
    for (size_t i = 0; i < chan.size(); ++i) chan[i] = (unsigned char)(i * 7);
    MUST(wfh5w_append(o, chan.data(), 20));
    MUST(wfh5w_set_attr_string(o, "TITLE", "channel map"));
    const std::vector<wfh5w_member> m = layout();
    MUST(wfh5w_create_table(o, "Records", m.data(), (int32_t)m.size(), ITEM));
    const int64_t cuts[] = {0, 1, 1000, 1024, 1025, 2048, ROWS};
    for (int i = 0; i + 1 < 7; ++i) MUST(wfh5w_append(o, rows.data() + cuts[i] * ITEM, cuts[i + 1] - cuts[i]));
    MUST(wfh5w_append(o, nullptr, 0));
    MUST(wfh5w_set_attr_string(o, "CLASS", "TABLE"));
    MUST(wfh5w_set_attr_string(o, "FIELD_0_NAME", "evt"));
    MUST(wfh5w_set_attr_string(o, "FIELD_1_NAME", "coord"));
    MUST(wfh5w_set_attr_string(o, "TITLE", "first title"));
    MUST(wfh5w_set_attr_string(o, "TITLE", "records"));          // replaced, not duplicated
    MUST(wfh5w_set_attr_f64(o, "nevents", 812.0));
    MUST(wfh5w_set_attr_f64(o, "abstime", 1.5e9));
    MUST(wfh5w_flush(o));
    // refusals on a healthy handle
    note(wfh5w_append(o, nullptr, 3));
    note(wfh5w_append(o, rows.data(), -1));
    const wfh5w_member bad[] = {mk("a", 0, WFH5W_I32, 2), mk("b", 4, WFH5W_I32, 1)};
    note(wfh5w_create_table(nullptr, "x", bad, 2, 12));
    MUST(wfh5w_close(o));
    // overlapping / outside / unnamed members are refused before anything is created
    MUST(wfh5w_create((path + ".bad").c_str(), &o));
    if (note(wfh5w_create_table(o, "x", bad, 2, 12)) == WFH5W_OK) return 1;
    const wfh5w_member outside[] = {mk("a", 8, WFH5W_F64, 1)};
    if (note(wfh5w_create_table(o, "x", outside, 1, 12)) == WFH5W_OK) return 1;
    const wfh5w_member kind[] = {mk("a", 0, 9, 1)};
    if (note(wfh5w_create_table(o, "x", kind, 1, 12)) == WFH5W_OK) return 1;
    if (note(wfh5w_append(o, rows.data(), 1)) == WFH5W_OK) return 1;          // no table
    if (note(wfh5w_set_attr_f64(o, "x", 1.0)) == WFH5W_OK) return 1;
    MUST(wfh5w_close(o));
    unlink((path + ".bad").c_str());
    return 0;
}

// every input entry point on one file; `expect`: the intact rows (nullptr for damaged files)
static int walk(const std::string &path, const std::vector<unsigned char> *expect, const std::string &copy_to) {
    for (const char *table : {"Records", "Chanmap", "no_such_table", "/"}) {
        wfh5w_in *in = nullptr;
        const int rc = note(wfh5w_open_input(path.c_str(), table, &in));
        if (rc != WFH5W_OK || !in) {
            if (expect && (!strcmp(table, "Records") || !strcmp(table, "Chanmap"))) return 1;
            continue;
        }
        if (expect && (!strcmp(table, "no_such_table") || !strcmp(table, "/"))) return 1;
        int64_t n = 0, item = 0;
        int32_t nm = 0;
        note(wfh5w_input_info(in, &n, &item, &nm));
        for (int32_t i = -1; i <= nm && i < 64; ++i) {
            wfh5w_member m;
            note(wfh5w_input_member(in, i, &m));
        }
        if (n >= 0 && n < (1 << 20) && item > 0 && item < (1 << 16)) {
            const int64_t spans[][2] = {{0, n}, {0, 1}, {n / 3, n / 3 + 7}, {1020, 1030}, {n - 1, n}, {n, n}, {0, n + 5}, {-1, 3}, {5, 2}};
            for (const auto &sp : spans) {
                const int64_t want = sp[1] > sp[0] ? sp[1] - sp[0] : 0;
                std::vector<unsigned char> buf((size_t)(want > 0 ? want : 1) * (size_t)item, 0xAB);
                const int r = note(wfh5w_read_records(in, sp[0], sp[1], buf.data(), buf.size()));
                if (expect && !strcmp(table, "Records")) {
                    const bool valid = sp[0] >= 0 && sp[1] >= sp[0] && sp[1] <= n;
                    if (valid != (r == WFH5W_OK)) return 1;
                    if (valid && want > 0 && memcmp(buf.data(), expect->data() + sp[0] * item, (size_t)(want * item)) != 0) {
                        fprintf(stderr, "h5writer_sanitize: rows [%lld, %lld) differ\n", (long long)sp[0], (long long)sp[1]);
                        return 1;
                    }
                }
                if (want > 1) note(wfh5w_read_records(in, sp[0], sp[1], buf.data(), buf.size() - 1));     // short buffer
            }
        }
        for (const char *a : {"CLASS", "TITLE", "FIELD_0_NAME", "nevents", "abstime", "nope"}) {
            char buf[64];
            int32_t is_str = 0;
            int64_t len = 0;
            const int r = note(wfh5w_read_attr(in, a, buf, sizeof(buf), &is_str, &len));
            note(wfh5w_read_attr(in, a, buf, 2, &is_str, &len));                                         // too small
            if (expect && !strcmp(table, "Records")) {
                if (!strcmp(a, "TITLE") && (r != WFH5W_OK || !is_str || strcmp(buf, "records"))) return 1;
                if (!strcmp(a, "nevents")) {
                    double v = 0;
                    memcpy(&v, buf, 8);
                    if (r != WFH5W_OK || is_str || len != 1 || v != 812.0) return 1;
                }
                if (!strcmp(a, "nope") && r == WFH5W_OK) return 1;
            }
        }
        if (!strcmp(table, "Records") && !copy_to.empty()) {
            // the writers' use: Chanmap, a table of the input's type, its attributes, the rows
            wfh5w_out *o = nullptr;
            if (note(wfh5w_create(copy_to.c_str(), &o)) == WFH5W_OK && o) {
                note(wfh5w_copy_dataset(o, in, "Chanmap"));
                note(wfh5w_copy_dataset(o, in, "nope"));
                if (note(wfh5w_create_table_like(o, in)) == WFH5W_OK) {
                    note(wfh5w_copy_table_attrs(o, in));
                    if (n > 0 && n < (1 << 20) && item > 0 && item < (1 << 16)) {
                        std::vector<unsigned char> buf((size_t)n * (size_t)item);
                        if (note(wfh5w_read_records(in, 0, n, buf.data(), buf.size())) == WFH5W_OK) {
                            note(wfh5w_append(o, buf.data(), n / 2));
                            note(wfh5w_append(o, buf.data() + (n / 2) * item, n - n / 2));
                        }
                    }
                    note(wfh5w_flush(o));
                }
                note(wfh5w_close(o));
            }
        }
        wfh5w_close_input(in);
    }
    return 0;
}

static void payload_ranges(const std::string &path, std::vector<std::pair<size_t, size_t>> *out) {
    H5Eset_auto2(H5E_DEFAULT, nullptr, nullptr);
    hid_t f = H5Fopen(path.c_str(), H5F_ACC_RDONLY, H5P_DEFAULT);
    if (f < 0) return;
    for (const char *table : {"Records", "Chanmap"}) {
        hid_t d = H5Dopen2(f, table, H5P_DEFAULT);
        if (d < 0) continue;
        hid_t space = H5Dget_space(d);
        hsize_t n = 0;
        if (space >= 0 && H5Dget_num_chunks(d, space, &n) >= 0)
            for (hsize_t i = 0; i < n; ++i) {
                hsize_t off[8];
                unsigned mask = 0;
                haddr_t addr = 0;
                hsize_t size = 0;
                if (H5Dget_chunk_info(d, space, i, off, &mask, &addr, &size) >= 0 && addr != HADDR_UNDEF && size > 0)
                    out->push_back({(size_t)addr, (size_t)size});
            }
        if (space >= 0) H5Sclose(space);
        H5Dclose(d);
    }
    H5Fclose(f);
}

static bool read_all(const std::string &path, std::vector<unsigned char> *out) {
    FILE *fp = fopen(path.c_str(), "rb");
    if (!fp) return false;
    fseek(fp, 0, SEEK_END);
    const long n = ftell(fp);
    fseek(fp, 0, SEEK_SET);
    out->resize((size_t)(n > 0 ? n : 0));
    const size_t got = n > 0 ? fread(out->data(), 1, (size_t)n, fp) : 0;
    fclose(fp);
    return got == out->size();
}

static bool write_all(const std::string &path, const unsigned char *p, size_t n) {
    FILE *fp = fopen(path.c_str(), "wb");
    if (!fp) return false;
    const size_t put = n ? fwrite(p, 1, n, fp) : 0;
    fclose(fp);
    return put == n;
}

int main(int argc, char **argv) {
    const std::string scratch = argc > 1 ? argv[1] : "/tmp";
    const std::string tag = scratch + "/wfh5w_sanitize_" + std::to_string((long)getpid());
    const std::string path = tag + ".h5", copy = tag + "_copy.h5", tmp = tag + "_damaged.h5", sink = tag + "_sink.h5";
    uint64_t lcg = 0x9E3779B97F4A7C15ull;
    auto rnd = [&]() {
        lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
        return (uint32_t)(lcg >> 33);
    };
    std::vector<unsigned char> rows((size_t)(ROWS * ITEM));
    for (size_t i = 0; i < rows.size(); ++i) rows[i] = (unsigned char)(rnd() % 7 == 0 ? rnd() : i / 97);   // compressible, not constant
    if (write_file(path, rows)) return 1;
    // the hole of a record is not part of any member: libhdf5 does not carry it.  Compare the members' bytes only.
    std::vector<unsigned char> expect = rows;
    {
        wfh5w_in *in = nullptr;
        MUST(wfh5w_open_input(path.c_str(), "Records", &in));
        MUST(wfh5w_read_records(in, 0, ROWS, expect.data(), expect.size()));
        wfh5w_close_input(in);
        for (int64_t r = 0; r < ROWS; ++r)
            if (memcmp(expect.data() + r * ITEM, rows.data() + r * ITEM, 50) != 0) {
                fprintf(stderr, "h5writer_sanitize: row %lld read back differs from what was written\n", (long long)r);
                return 1;
            }
    }
    if (walk(path, &expect, copy)) {
        fprintf(stderr, "h5writer_sanitize: the intact file did not read back as written (%s)\n", wfh5w_last_error());
        return 1;
    }
    if (walk(copy, &expect, "")) {
        fprintf(stderr, "h5writer_sanitize: the copy differs from its source (%s)\n", wfh5w_last_error());
        return 1;
    }
    std::vector<unsigned char> bytes;
    if (!read_all(path, &bytes) || bytes.size() < 64) return 1;
    long damaged = 0, flipped = 0;
    const size_t cuts[] = {bytes.size() - 1, bytes.size() * 3 / 4, bytes.size() / 2, 2048, 9};
    for (size_t cut : cuts) {
        if (cut >= bytes.size() || !write_all(tmp, bytes.data(), cut)) continue;
        walk(tmp, nullptr, sink);
        ++damaged;
    }
    std::vector<std::pair<size_t, size_t>> ranges;
    payload_ranges(path, &ranges);
    size_t payload = 0;
    for (const auto &r : ranges) payload += r.second;
    for (int round = 0; round < 24 && payload > 0; ++round) {
        std::vector<unsigned char> b = bytes;
        const int flips = 1 + (int)(rnd() % 8);
        for (int i = 0; i < flips; ++i) {
            size_t k = rnd() % payload, at = 0;
            for (const auto &r : ranges) {
                if (k < r.second) {
                    at = r.first + (rnd() % 3 == 0 ? rnd() % (r.second < 16 ? r.second : 16) : k);
                    break;
                }
                k -= r.second;
            }
            if (at >= b.size()) continue;
            b[at] ^= (unsigned char)(1u << (rnd() % 8));
            if (rnd() % 4 == 0) b[at] = (unsigned char)rnd();
            ++flipped;
        }
        if (!write_all(tmp, b.data(), b.size())) continue;
        walk(tmp, nullptr, sink);
        ++damaged;
    }
    for (const std::string &p : {path, copy, tmp, sink}) unlink(p.c_str());
    printf("h5writer_sanitize: %lld rows round trip, %ld damaged copies (%ld payload bytes flipped), %ld calls (%ld ok, %ld refused), "
           "last error: %s\n", (long long)ROWS, damaged, flipped, g_calls, g_ok, g_failed, wfh5w_last_error());
    return 0;
}
