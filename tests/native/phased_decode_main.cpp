// Stand-alone check of the host side of matrix.snp_phased_ancestry (adelie_amd/csrc/phased_decode_host.hpp), built with
// -fsanitize=address,undefined by tests/test_phased_host.py.
//
//   phased_decode_main image.bin table.bin calldata.bin ancestries.bin
//
// image.bin is a valid phased-ancestry .snpdat image, table.bin the code table numpy expects from it (column-major uint8
// (n, 2 s): the ancestry of a mutation, 255 elsewhere), calldata.bin / ancestries.bin the column-major int8 (n, 2 s) arrays
// the image was written from.  The program decodes the image and packs the pair, compares both with the table, then damages
// copies of the image -- each in a heap block of exactly its length, so that a read past the end is the sanitizer's -- and
// requires the error return for every one: truncations, an outer entry / a haplotype offset past the end, a chunk whose count
// byte overruns its block, a chunk index past the rows, A = 0.  The last haplotype block of the image must end in a chunk of
// fewer than 256 rows (the test's data sees to it).  Exits non-zero on the first disagreement.
#include "../../adelie_amd/csrc/phased_decode_host.hpp"
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

// header + decode as the library calls them; the message of the first failure, nullptr for a clean decode
static const char* decode(const std::vector<uint8_t>& img, std::vector<uint8_t>* table, PhasedDims* dims) {
    const uint8_t* p = img.empty() ? nullptr : img.data();
    if (const char* e = phased_header(p, img.size(), dims)) return e;
    table->assign(size_t(dims->n) * size_t(2 * dims->s), 0);
    return phased_decode(p, img.size(), *dims, table->data());
}

static void must_fail(const char* what, const std::vector<uint8_t>& img) {
    std::vector<uint8_t> exact(img.begin(), img.end()); // capacity == size: the redzone starts at the last byte
    exact.shrink_to_fit();
    std::vector<uint8_t> table;
    PhasedDims d;
    const char* e = decode(exact, &table, &d);
    std::printf("%-40s -> %s\n", what, e ? e : "(decoded)");
    if (!e) { std::printf("FAILED: %s decoded without an error\n", what); ++fails; }
}

static void put_u64(std::vector<uint8_t>& v, size_t at, uint64_t x) { std::memcpy(v.data() + at, &x, 8); }
static void put_u32(std::vector<uint8_t>& v, size_t at, uint32_t x) { std::memcpy(v.data() + at, &x, 4); }

int main(int argc, char** argv) {
    if (argc != 5) { std::printf("usage: %s image table calldata ancestries\n", argv[0]); return 2; }
    const std::vector<uint8_t> img = slurp(argv[1]), want = slurp(argv[2]), cal = slurp(argv[3]), anc = slurp(argv[4]);

    // the valid image, and the same table from the pair it was written from
    std::vector<uint8_t> table;
    PhasedDims d;
    const char* e = decode(img, &table, &d);
    CHECK(e == nullptr);
    if (e) { std::printf("valid image: %s\n", e); return 1; }
    const uint64_t n = d.n, s = d.s, A = d.A;
    std::printf("n=%llu s=%llu A=%llu bytes=%zu\n", (unsigned long long)n, (unsigned long long)s, (unsigned long long)A, img.size());
    CHECK(table.size() == want.size() && table == want);
    CHECK(cal.size() == want.size() && anc.size() == want.size());
    if (fails) return 1;
    const int8_t* calp = reinterpret_cast<const int8_t*>(cal.data());
    const int8_t* ancp = reinterpret_cast<const int8_t*>(anc.data());
    std::vector<uint8_t> packed(want.size(), 0);
    CHECK(phased_pack_dims(int64_t(n), int64_t(s), int64_t(A)) == nullptr);
    CHECK(phased_pack(calp, ancp, int64_t(n), int64_t(s), int64_t(A), packed.data()) == nullptr);
    CHECK(packed == want);
    {   // the writer's errors of the pair
        std::vector<uint8_t> bad = anc;
        bad[bad.size() / 2] = uint8_t(A);
        CHECK(phased_pack(calp, reinterpret_cast<const int8_t*>(bad.data()), int64_t(n), int64_t(s), int64_t(A), packed.data()) != nullptr);
        bad = anc;
        bad[0] = uint8_t(-1);
        CHECK(phased_pack(calp, reinterpret_cast<const int8_t*>(bad.data()), int64_t(n), int64_t(s), int64_t(A), packed.data()) != nullptr);
        bad = cal;
        bad[bad.size() - 1] = 2;
        CHECK(phased_pack(reinterpret_cast<const int8_t*>(bad.data()), ancp, int64_t(n), int64_t(s), int64_t(A), packed.data()) != nullptr);
        CHECK(phased_pack_dims(int64_t(n), int64_t(s), 256) != nullptr && phased_pack_dims(int64_t(n), int64_t(s), 0) != nullptr);
        CHECK(phased_pack_dims(0, int64_t(s), int64_t(A)) != nullptr && phased_pack_dims(int64_t(1) << 31, 1, 1) != nullptr);
        CHECK(phased_pack_dims(5, (int64_t(1) << 31) / 4, 4) != nullptr);
    }

    // where things lie in the (valid) image
    const size_t outer_at = 18 + 16 * s * A, hdr = d.header_bytes();
    const uint64_t last_base = phased_read_u64(img.data() + outer_at + 8 * (s - 1));
    const uint64_t last_ablk = last_base + phased_read_u64(img.data() + last_base + 8 * (A - 1));
    uint64_t pos = last_ablk + phased_read_u64(img.data() + last_ablk + 8);
    const uint32_t n_chunks = phased_read_u32(img.data() + pos);
    CHECK(n_chunks >= 1);
    if (fails) return 1;
    pos += 4;
    for (uint32_t c = 0; c + 1 < n_chunks; ++c) pos += 5 + uint64_t(img[pos + 4]) + 1;
    const size_t last_chunk = size_t(pos); // [u32 chunk_idx][u8 nnz-1][rows], the last bytes of the image
    CHECK(last_chunk + 5 + size_t(img[last_chunk + 4]) + 1 == img.size());
    CHECK(img[last_chunk + 4] < 255);
    if (fails) return 1;

    // damages
    const size_t cuts[] = {0, 1, 9, 17, 18, 19, hdr - 8, hdr - 1, hdr, hdr + 1, hdr + 8 * size_t(A) - 1, hdr + 8 * size_t(A), hdr + 8 * size_t(A) + 15,
                           size_t(last_base), size_t(last_ablk) + 7, last_chunk, last_chunk + 4, last_chunk + 5, img.size() / 2, img.size() - 1};
    for (size_t cut : cuts) {
        if (cut >= img.size()) continue;
        must_fail(("truncated at " + std::to_string(cut)).c_str(), std::vector<uint8_t>(img.begin(), img.begin() + cut));
    }
    {
        std::vector<uint8_t> v = img;
        put_u64(v, outer_at + 8 * s, img.size() + 1);
        must_fail("outer[s] past the end", v);
        v = img;
        put_u64(v, outer_at, ~uint64_t(0) - 3);
        must_fail("outer[0] huge", v);
        v = img;
        put_u64(v, outer_at, hdr - 1);
        must_fail("outer[0] inside the header", v);
    }
    {
        std::vector<uint8_t> v = img;
        put_u64(v, size_t(last_ablk) + 8, img.size());
        must_fail("hap_off[1] past the end", v);
        v = img;
        put_u64(v, size_t(last_ablk) + 8, ~uint64_t(0));
        must_fail("hap_off[1] huge", v);
        v = img;
        put_u64(v, size_t(last_base) + 8 * (A - 1), img.size() - last_base - 15);
        must_fail("anc_off[A-1] too close to the end", v);
    }
    {
        std::vector<uint8_t> v = img;
        v[last_chunk + 4] = 255;
        must_fail("chunk count byte raised", v);
        v = img;
        put_u32(v, size_t(last_ablk + phased_read_u64(img.data() + last_ablk + 8)), n_chunks + 1);
        must_fail("one chunk too many", v);
        v = img;
        put_u32(v, last_chunk, uint32_t((n + kPhasedChunk - 1) / kPhasedChunk));
        must_fail("chunk_idx past the rows", v);
        v = img;
        put_u32(v, last_chunk, 0xffffffffu);
        must_fail("chunk_idx 2^32 - 1", v);
    }
    {
        std::vector<uint8_t> v = img;
        v[17] = 0;
        must_fail("A = 0", v);
        v = img;
        v[0] = 1;
        must_fail("big-endian flag", v);
        v = img;
        put_u64(v, 9, ~uint64_t(0) / 2);
        must_fail("s huge", v);
        v = img;
        put_u64(v, 1, uint64_t(1) << 31);
        must_fail("n = 2^31", v);
    }
    if (fails) return 1;
    std::printf("phased_decode: ok\n");
    return 0;
}
