// design_snp.hpp — part of design.hip, which includes it inside its extern "C" block (one translation unit, several readable
// files): the constructors of a 2-bit SNP design (int8 calldata, an unphased .snpdat image, a PLINK .bed image) and what they share.

// (snp_alloc_bits / snp_alloc_impute: design.hip, next to alloc_dense)
// The columns go through a temporary device block in panels that bound it by 2^28 bytes (or one column) where a column takes
// col_bytes there: stage(j0, pc, tmp) fills the block for columns [j0, j0 + pc) and launches their transcode on d->stream.
static void snp_for_each_panel(adelie_hip_design* d, int64_t col_bytes, const std::function<void(int64_t, int64_t, void*)>& stage) {
    const int64_t p = d->p, panel = std::min(p, std::max<int64_t>(1, (int64_t(1) << 28) / col_bytes));
    DevTmp tmp;
    tmp.alloc(size_t(col_bytes) * size_t(panel));
    for (int64_t j0 = 0; j0 < p; j0 += panel) {
        stage(j0, std::min(panel, p - j0), tmp);
        AHIP_CHECK(hipStreamSynchronize(d->stream));
    }
}

static void upload_impute(adelie_hip_design* d, const double* impute) {
    const size_t p = size_t(d->p);
    snp_alloc_impute(d);
    if (d->dtype == ADELIE_HIP_F64) {
        AHIP_CHECK(hipMemcpy(d->impute, impute, p * sizeof(double), hipMemcpyHostToDevice));
    } else {
        std::vector<float> f(impute, impute + p);
        AHIP_CHECK(hipMemcpy(d->impute, f.data(), p * sizeof(float), hipMemcpyHostToDevice));
    }
}

int adelie_hip_design_create_snp_calldata(const int8_t* calldata, int64_t n, int64_t p, const double* impute, int dtype,
                                          int device, adelie_hip_design** out) {
    ABI_TRY
    if (!calldata || !impute || !out) throw make_core_error("null argument.");
    DesignGuard g(new_design(n, p, dtype, device));
    adelie_hip_design* d = g.get();
    snp_alloc_bits(d);
    snp_for_each_panel(d, n, [&](int64_t j0, int64_t pc, void* tmp) {
        // hipMemcpyDefault: the calldata may live on the host or (generated in place) on this device
        AHIP_CHECK(hipMemcpyAsync(tmp, calldata + j0 * n, size_t(n) * size_t(pc), hipMemcpyDefault, d->stream));
        launch_pack_snp(static_cast<const int8_t*>(tmp), n, pc, d->bits + j0 * d->ldb, d->ldb, d->stream);
    });
    upload_impute(d, impute);
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_snp_unphased(const void* snpdat, int64_t n_bytes, int dtype, int device,
                                          adelie_hip_design** out) {
    ABI_TRY
    if (!snpdat || !out) throw make_core_error("null argument.");
    const uint8_t* buf = static_cast<const uint8_t*>(snpdat);
    // (whatever the header claims, the host never holds more than one panel of decoded columns, 256 MB or one column, and the
    // packed matrix is allocated on the device BEFORE any decoding: an image whose counts were damaged fails there)
    SnpUnphasedDims dims;
    if (const char* e = snp_unphased_header(buf, n_bytes < 0 ? 0 : uint64_t(n_bytes), &dims)) throw make_core_error(e);
    const int64_t n = int64_t(dims.n), p = int64_t(dims.p);
    const uint8_t* outer_p = buf + dims.outer_at();
    std::vector<double> impute(dims.p);
    std::memcpy(impute.data(), buf + dims.impute_at(), 8 * dims.p);
    DesignGuard g(new_design(n, p, dtype, device));
    adelie_hip_design* d = g.get();
    snp_alloc_bits(d);
    // decode -> int8 panel on the host -> 2-bit on the device, a panel of columns at a time
    std::vector<int8_t> calls;
    snp_for_each_panel(d, n, [&](int64_t j0, int64_t pc, void* tmp) {
        calls.assign(size_t(n) * size_t(pc), int8_t(0)); // (the first panel is the largest: allocated once)
        for (int64_t j = j0; j < j0 + pc; ++j)
            if (const char* e = snp_unphased_decode_column(buf, phased_read_u64(outer_p + 8 * j), phased_read_u64(outer_p + 8 * (j + 1)),
                                                           dims.n, calls.data() + size_t(j - j0) * size_t(n)))
                throw make_core_error(e);
        AHIP_CHECK(hipMemcpyAsync(tmp, calls.data(), size_t(n) * size_t(pc), hipMemcpyHostToDevice, d->stream));
        launch_pack_snp(static_cast<const int8_t*>(tmp), n, pc, d->bits + j0 * d->ldb, d->ldb, d->stream);
    });
    upload_impute(d, impute.data());
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_snp_bed(const void* bed, int64_t n_bytes, int64_t n, int64_t p, int dtype, int device,
                                     adelie_hip_design** out) {
    ABI_TRY
    if (!bed || !out) throw make_core_error("null argument.");
    if (n <= 0 || p <= 0) throw make_core_error("n and p must be positive.");
    const uint8_t* buf = static_cast<const uint8_t*>(bed);
    const int64_t stride = (n + 3) / 4;
    if (n_bytes < 3 || buf[0] != 0x6c || buf[1] != 0x1b) throw make_core_error("not a PLINK .bed image (bad magic).");
    if (buf[2] != 0x01) throw make_core_error("only SNP-major .bed files (third byte 0x01) are supported.");
    if (n_bytes < 3 + stride * p) throw make_core_error("truncated .bed image: expected 3 + ceil(n/4)*p bytes.");
    DesignGuard g(new_design(n, p, dtype, device));
    adelie_hip_design* d = g.get();
    snp_alloc_bits(d);
    snp_for_each_panel(d, stride, [&](int64_t j0, int64_t pc, void* tmp) {
        AHIP_CHECK(hipMemcpyAsync(tmp, buf + 3 + j0 * stride, size_t(stride) * size_t(pc), hipMemcpyDefault, d->stream));
        launch_bed_transcode(static_cast<const uint8_t*>(tmp), n, pc, stride, d->bits + j0 * d->ldb, d->ldb, d->stream);
    });
    snp_alloc_impute(d);
    DTYPE_DISPATCH(d, launch_snp_impute<T>(d->bits, n, p, d->ldb, static_cast<T*>(d->impute), d->stream))
    AHIP_CHECK(hipStreamSynchronize(d->stream));
    *out = g.release();
    ABI_CATCH
}
