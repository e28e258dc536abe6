// Stand-alone check of the unphased .snpdat reader (adelie_amd/csrc/snp_decode_host.hpp), built with
// -fsanitize=address,undefined by tests/test_snp_decode_host.py.
//
//   snp_decode_main image.bin calls.bin
//
// image.bin is a valid unphased .snpdat image, calls.bin the column-major int8 (n, p) matrix it was written from (missing = -9).
// The program decodes the image as adelie_hip_design_create_snp_unphased does and compares, then damages copies of the image
// -- each in a heap block of exactly its length, so that a read past the end is the sanitizer's -- and requires the error
// return for every directed one: truncations, an outer entry past the end / huge / inside the header, a category offset too
// close to its column's end, a raised count byte, one chunk too many, a chunk index past the rows, n = 2^45.  A sweep of
// single-byte damages over the header and the first column's tables follows: not every one of those makes the image invalid,
// so they are counted.  Category 2 of the last column must end in a chunk of fewer than 256 rows (the test's data sees to
// it).  Exits non-zero on the first disagreement.
#include "../../adelie_amd/csrc/snp_decode_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

using namespace ahip;

static int fails = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED line %d: %s\n", __LINE__, #c); ++fails; } } while (0)

static std::vector<uint8_t> slurp(const char* path) {
    std::vector<uint8_t> out;
    std::FILE* f = std::fopen(path, "rb");
    if (!f) { std::printf("cannot open %s\n", path); std::exit(2); }
    uint8_t buf[4096];
    for (size_t k; (k = std::fread(buf, 1, sizeof buf, f)) > 0;) out.insert(out.end(), buf, buf + k);
    std::fclose(f);
    return out;
}

// header + columns as the library calls them, one column at a time; `want` (n * p calls), when given, is compared.  The
// message of the first failure, nullptr for a clean decode.
static const char* decode(const std::vector<uint8_t>& img, SnpUnphasedDims* dims, const std::vector<uint8_t>* want = nullptr) {
    const uint8_t* buf = img.empty() ? nullptr : img.data();
    if (const char* e = snp_unphased_header(buf, img.size(), dims)) return e;
    const uint8_t* outer = buf + dims->outer_at();
    std::vector<int8_t> col(size_t(dims->n));
    if (want) CHECK(want->size() == size_t(dims->n) * size_t(dims->p));
    for (uint64_t j = 0; j < dims->p; ++j) {
        col.assign(size_t(dims->n), 0);
        if (const char* e = snp_unphased_decode_column(buf, phased_read_u64(outer + 8 * j), phased_read_u64(outer + 8 * (j + 1)), dims->n, col.data()))
            return e;
        if (want && !fails) CHECK(std::memcmp(col.data(), want->data() + size_t(j) * size_t(dims->n), size_t(dims->n)) == 0);
    }
    return nullptr;
}

static const char* attempt(const std::vector<uint8_t>& img) {
    std::vector<uint8_t> exact(img.begin(), img.end()); // capacity == size: the redzone starts at the last byte
    exact.shrink_to_fit();
    SnpUnphasedDims d;
    return decode(exact, &d);
}
static void must_fail(const char* what, const std::vector<uint8_t>& img) {
    const char* e = attempt(img);
    std::printf("%-40s -> %s\n", what, e ? e : "(decoded)");
    if (!e) { std::printf("FAILED: %s decoded without an error\n", what); ++fails; }
}

static void put_u64(std::vector<uint8_t>& v, size_t at, uint64_t x) { std::memcpy(v.data() + at, &x, 8); }
static void put_u32(std::vector<uint8_t>& v, size_t at, uint32_t x) { std::memcpy(v.data() + at, &x, 4); }

int main(int argc, char** argv) {
    if (argc != 3) { std::printf("usage: %s image calls\n", argv[0]); return 2; }
    const std::vector<uint8_t> img = slurp(argv[1]), want = slurp(argv[2]);

    SnpUnphasedDims d;
    const char* e = decode(img, &d, &want);
    CHECK(e == nullptr);
    if (e) { std::printf("valid image: %s\n", e); return 1; }
    if (fails) return 1;
    const uint64_t n = d.n, p = d.p;
    std::printf("n=%llu p=%llu bytes=%zu\n", (unsigned long long)n, (unsigned long long)p, img.size());

    // where things lie in the (valid) image
    const size_t outer_at = size_t(d.outer_at()), hdr = size_t(d.header_bytes());
    const uint64_t base0 = phased_read_u64(img.data() + outer_at);
    const uint64_t last_base = phased_read_u64(img.data() + outer_at + 8 * (p - 1));
    CHECK(base0 == hdr && phased_read_u64(img.data() + outer_at + 8 * p) == img.size());
    const size_t last_cat = size_t(last_base + phased_read_u64(img.data() + last_base + 16)); // [u32 n_chunks] of category 2
    const uint32_t n_chunks = phased_read_u32(img.data() + last_cat);
    CHECK(n_chunks >= 1);
    if (fails) return 1;
    size_t pos = last_cat + 4;
    for (uint32_t c = 0; c + 1 < n_chunks; ++c) pos += 5 + size_t(img[pos + 4]) + 1;
    const size_t last_chunk = pos; // [u32 chunk_idx][u8 nnz-1][rows], the last bytes of the image
    CHECK(last_chunk + 5 + size_t(img[last_chunk + 4]) + 1 == img.size());
    CHECK(img[last_chunk + 4] < 255);
    if (fails) return 1;

    // directed damages
    const size_t cuts[] = {0, 1, 5, 9, 16, 17, hdr - 8, hdr - 1, hdr, hdr + 1, hdr + 10, hdr + 23, hdr + 24, hdr + 27, hdr + 28, hdr + 32, hdr + 33,
                           size_t(last_base), size_t(last_base) + 23, last_cat, last_cat + 3, last_chunk, last_chunk + 4, last_chunk + 5,
                           img.size() / 2, img.size() - 1};
    for (size_t cut : cuts) {
        if (cut >= img.size()) continue;
        must_fail(("truncated at " + std::to_string(cut)).c_str(), std::vector<uint8_t>(img.begin(), img.begin() + cut));
        if (cut < last_base) continue;
        // (the column index alone refuses a plain truncation; with outer[p] moved to the cut, the checks inside the last column
        // -- its offset table, a category's chunk count, a chunk header, a chunk's rows -- have to)
        std::vector<uint8_t> v(img.begin(), img.begin() + cut);
        put_u64(v, outer_at + 8 * p, cut);
        must_fail(("cut and re-indexed at " + std::to_string(cut)).c_str(), v);
    }
    {
        std::vector<uint8_t> v = img;
        put_u64(v, outer_at + 8 * p, img.size() + 1);
        must_fail("outer[p] past the end", v);
        v = img;
        put_u64(v, outer_at, ~uint64_t(0) - 3);
        must_fail("outer[0] huge", v);
        v = img;
        put_u64(v, outer_at, hdr - 1);
        must_fail("outer[0] inside the header", v);
    }
    for (uint64_t back = 0; back <= 3; ++back) {
        std::vector<uint8_t> v = img;
        put_u64(v, size_t(last_base) + 16, img.size() - last_base - back);
        must_fail(("cat_off[2] " + std::to_string(back) + " bytes before the column's end").c_str(), v);
    }
    {
        std::vector<uint8_t> v = img;
        put_u64(v, size_t(last_base) + 16, ~uint64_t(0));
        must_fail("cat_off[2] huge", v);
        v = img;
        v[last_chunk + 4] = 255;
        must_fail("chunk count byte raised", v);
        v = img;
        put_u32(v, last_cat, n_chunks + 1);
        must_fail("one chunk too many", v);
        v = img;
        put_u32(v, last_chunk, uint32_t((n + kSnpChunk - 1) / kSnpChunk));
        must_fail("chunk_idx past the rows", v);
        v = img;
        put_u32(v, last_chunk, 0xffffffffu);
        must_fail("chunk_idx 2^32 - 1", v);
        v = img;
        put_u64(v, 1, uint64_t(1) << 45);
        const char* msg = attempt(v);
        must_fail("n = 2^45", v);
        CHECK(msg && std::string(msg).find("row / column counts") != std::string::npos);
        v = img;
        put_u64(v, 9, ~uint64_t(0) / 2);
        must_fail("p huge", v);
        v = img;
        put_u64(v, 9, 0);
        must_fail("p = 0", v);
    }

    // Every byte of the header and of the first column's offset table / chunk headers damaged in turn.  Byte 4 is left alone: it
    // turns n into ~4e9 rows, still below the plausibility cap (2^32), which would only make this program allocate gigabytes
    // for a "valid" all-zero tail.
    int n_rejected = 0, n_tried = 0;
    std::vector<size_t> at;
    for (size_t q = 1; q < 17; ++q)
        if (q != 4) at.push_back(q);
    for (size_t q = outer_at; q < hdr + 40 && q < img.size(); ++q) at.push_back(q);
    for (size_t q : at)
        for (int val : {0xFF, 0x00, 0x7F}) {
            if (img[q] == uint8_t(val)) continue;
            std::vector<uint8_t> v = img;
            v[q] = uint8_t(val);
            ++n_tried;
            n_rejected += attempt(v) != nullptr;
        }
    std::printf("byte sweep: %d of %d rejected\n", n_rejected, n_tried);
    CHECK(n_rejected > 50);
    if (fails) return 1;
    std::printf("snp_decode: ok\n");
    return 0;
}
