// design_csc.hpp — part of design.hip, which includes it inside its extern "C" block (one translation unit, several readable
// files): the designs kept sparse.  csc_finish, csc_alloc and csc_build_from_counts are what the constructors share.

// The second half of every constructor of a design kept sparse, from the point where the six compressed arrays lie in device
// memory (d->kind, d->nnz set; the copies or kernels that fill them enqueued on d->stream): the row-block pointers and the
// tile-major copy for the full sweeps.
static void csc_finish(adelie_hip_design* d) {
    const int64_t n = d->n, p = d->p, nnz = d->nnz;
    const size_t vs = d->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    const size_t nz1 = size_t(std::max<int64_t>(nnz, 1));
    hipStream_t s = d->stream;
    csc_block_layout(n, vs, &d->sp_nb, &d->sp_rb);
    if (d->sp_nb > 1) {
        d->bptr.alloc(size_t(p) * size_t(d->sp_nb + 1));
        launch_csc_block_ptr(d->cptr, d->cidx, p, d->sp_nb, d->sp_rb, d->bptr, s);
    }
    // Tile-major copy for the full sweeps (csc_tile_sweep_kernel): tiles of kCscTileBytes of an n-vector.  Built on the
    // device from the per-column tile pointers; the tile-major offsets are a prefix sum over (tile, column) on the host.
    const int64_t th = kCscTileBytes / int64_t(vs);
    const int64_t nt = (n + th - 1) / th;
    // (the tile of v is 128 KB of dynamic LDS — gfx950 has 160 KB per workgroup, the only target of this library; a launch
    // the device refuses raises in raw_sweep)
    const bool worth = nt > 1 && nt <= 4096 && nnz >= (int64_t(1) << 16) && nt * (p + 1) * 8 <= (int64_t(1) << 30) &&
                       nnz / (nt * p) >= 4; // (segments of a few entries at least: below, the pointers outweigh the entries)
    if (worth) {
        DevArr<int64_t> colptr;
        colptr.alloc(size_t(p) * size_t(nt + 1));
        launch_csc_block_ptr(d->cptr, d->cidx, p, int(nt), th, colptr, s);
        std::vector<int64_t> cp(size_t(p) * size_t(nt + 1)), tp(size_t(nt) * size_t(p + 1));
        AHIP_CHECK(hipMemcpyAsync(cp.data(), colptr, cp.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        AHIP_CHECK(hipStreamSynchronize(s));
        int64_t run = 0;
        for (int64_t t = 0; t < nt; ++t) {
            int64_t* row = tp.data() + size_t(t) * size_t(p + 1);
            for (int64_t c = 0; c < p; ++c) {
                row[c] = run;
                run += cp[size_t(c) * size_t(nt + 1) + size_t(t) + 1] - cp[size_t(c) * size_t(nt + 1) + size_t(t)];
            }
            row[p] = run;
        }
        d->tptr.alloc(tp.size()), d->trow.alloc(nz1), d->tval.alloc(nz1 * vs);
        AHIP_CHECK(hipMemcpyAsync(d->tptr, tp.data(), tp.size() * sizeof(int64_t), hipMemcpyHostToDevice, s));
        DTYPE_DISPATCH(d, launch_csc_tile_scatter<T>(colptr, d->cidx, static_cast<const T*>(d->cval), p, int(nt), th, d->tptr, d->trow,
                                                     static_cast<T*>(d->tval), s))
        AHIP_CHECK(hipStreamSynchronize(s));
        d->sp_nt = int(nt);
        d->sp_th = th;
    }
}

// d becomes a design kept sparse of `nnz` entries: the six compressed arrays for (d->n, d->p), the two pointer arrays first, then
// the four that grow with nnz.  With `what` (a constructor's name and ": ") a refusal of one of the four names the size that did not fit.
static void csc_alloc(adelie_hip_design* d, int64_t nnz, const char* what) {
    d->kind = adelie_hip_design::kCsc;
    d->nnz = nnz;
    const size_t vs = d->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    const size_t nz1 = size_t(std::max<int64_t>(nnz, 1));
    d->cptr.alloc(size_t(d->p + 1)), d->rptr.alloc(size_t(d->n + 1));
    if (!what) d->cidx.alloc(nz1), d->cval.alloc(nz1 * vs), d->rcol.alloc(nz1), d->rval.alloc(nz1 * vs);
    else if (!(d->cidx.try_alloc(nz1) && d->cval.try_alloc(nz1 * vs) && d->rcol.try_alloc(nz1) && d->rval.try_alloc(nz1 * vs)))
        throw make_core_error(std::string(what) + "could not allocate the expanded design (" + std::to_string(d->n) + " x " +
                              std::to_string(d->p) + ", " + std::to_string(nnz) + " stored entries) on the device.");
}

// The tail of a device build (d->p == cols_out): count(ccnt, rcnt) enqueues the kernels that count the entries per
// (column, tile) of the first cols_counted columns and per row, the counts are summed on the host (csc_build_host.hpp) into
// cptr, the segment starts and rptr, the six arrays are allocated, and fill(col_pos) enqueues the kernels that write them in the
// canonical form adelie_hip_design_create_csc demands of its caller.  `prefix` (the constructor's name and ": ") opens the
// messages; `oom_what` goes to csc_alloc.
static void csc_build_from_counts(adelie_hip_design* d, int64_t cols_counted, int64_t cols_out, int nt,
                                  const std::function<void(int32_t*, int64_t*)>& count, const std::function<void(const int64_t*)>& fill,
                                  const char* prefix, const char* oom_what) {
    const int64_t n = d->n;
    hipStream_t st = d->stream;
    const size_t segs = size_t(cols_counted) * size_t(nt), psegs = size_t(cols_out) * size_t(nt);
    DevArr<int32_t> ccnt;
    DevArr<int64_t> rcnt, cpos;
    ccnt.alloc(segs), rcnt.alloc(size_t(n));
    count(ccnt, rcnt);
    AHIP_CHECK(hipGetLastError());
    std::vector<int32_t> col_cnt(segs);
    std::vector<int64_t> col_pos(psegs), cptr(size_t(cols_out) + 1), rptr(size_t(n) + 1);
    AHIP_CHECK(hipMemcpyAsync(col_cnt.data(), ccnt, segs * sizeof(int32_t), hipMemcpyDeviceToHost, st));
    AHIP_CHECK(hipMemcpyAsync(rptr.data() + 1, rcnt, size_t(n) * sizeof(int64_t), hipMemcpyDeviceToHost, st));
    AHIP_CHECK(hipStreamSynchronize(st));
    int64_t nnz = 0;
    if (const char* e = csc_offsets_from_counts(col_cnt.data(), cols_counted, cols_out, nt, rptr.data() + 1, n, cptr.data(), col_pos.data(), rptr.data(), &nnz))
        throw make_core_error(std::string(prefix) + e);
    csc_alloc(d, nnz, oom_what);
    cpos.alloc(psegs);
    AHIP_CHECK(hipMemcpyAsync(d->cptr, cptr.data(), cptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AHIP_CHECK(hipMemcpyAsync(d->rptr, rptr.data(), rptr.size() * sizeof(int64_t), hipMemcpyHostToDevice, st));
    AHIP_CHECK(hipMemcpyAsync(cpos, col_pos.data(), psegs * sizeof(int64_t), hipMemcpyHostToDevice, st));
    fill(cpos);
    AHIP_CHECK(hipGetLastError());
    AHIP_CHECK(hipStreamSynchronize(st)); // (the counts, the segment starts and the caller's own temporaries are freed on the way out)
    csc_finish(d);
    AHIP_CHECK(hipStreamSynchronize(st));
}

// A phased-ancestry design from its host code table (phased_decode_host.hpp): the table is uploaded (2 n s bytes) and
// kernels_phased.hip counts and fills the entries around csc_build_from_counts.
static void phased_build(adelie_hip_design* d, const uint8_t* table, int64_t s, int A) {
    const int64_t n = d->n;
    const int nt = phased_tiles(n);
    if (s * int64_t(nt) >= (int64_t(1) << 31)) throw make_core_error("snp_phased_ancestry: too many (SNP, row tile) pairs.");
    hipStream_t st = d->stream;
    DevArr<uint8_t> code;
    code.alloc(size_t(n) * size_t(2 * s));
    const uint8_t* dcode = code;
    AHIP_CHECK(hipMemcpyAsync(code, table, size_t(n) * size_t(2 * s), hipMemcpyHostToDevice, st));
    csc_build_from_counts(
        d, d->p, d->p, nt, [&](int32_t* ccnt, int64_t* rcnt) { launch_phased_count(dcode, n, s, A, ccnt, rcnt, st); },
        [&](const int64_t* cpos) {
            DTYPE_DISPATCH(d, launch_phased_fill<T>(dcode, n, s, A, cpos, d->rptr, d->cidx, static_cast<T*>(d->cval), d->rcol,
                                                    static_cast<T*>(d->rval), st))
        },
        "snp_phased_ancestry: ", nullptr);
}

// A convex-relu design over the kept-sparse Z, kept sparse itself (kernels_relu_sparse.hip): Z's compressed columns are copied
// and cut at the row tiles, the host's column-major (n, m) mask bytes are uploaded and packed to words, and the entries are
// counted and filled around csc_build_from_counts (the signed half repeats the counts of the first).  The copy of Z and the mask
// words stay with the handle for the structured sweep.
static void relu_csc_build(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out) {
    const int64_t n = Z->n, dz = Z->p, znnz = Z->nnz;
    const size_t vs = Z->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    const double cols = double(gated ? 1 : 2) * double(m) * double(dz);
    if (cols > double((int64_t(1) << 31) - 64))
        throw make_core_error("convex_relu(): the expanded design has more columns than the solver's 32-bit column indices address (" +
                              std::to_string(double(gated ? 1 : 2) * double(m) * double(znnz)) + " stored entries at most).");
    const int64_t P = int64_t(cols), md = m * dz;
    const ReluSparseShape sh = relu_sparse_shape(n, m);
    const int nt = int(sh.tiles);
    if (dz * sh.tiles >= (int64_t(1) << 31) || sh.words > 65535)
        throw make_core_error("convex_relu(): too many (column of mat, row tile) pairs or mask columns for one launch.");
    DesignGuard g(new_design(n, P, Z->dtype, Z->device));
    adelie_hip_design* d = g.get();
    hipStream_t st = d->stream;
    d->r_d = dz;
    d->r_m = m;
    d->r_gated = gated ? 1 : 0;
    d->rz_nnz = znnz;
    const size_t zn1 = size_t(std::max<int64_t>(znnz, 1));
    d->rz_seg.alloc(size_t(dz) * size_t(nt + 1)), d->rz_idx.alloc(zn1), d->rz_val.alloc(zn1 * vs);
    d->rbits.alloc(size_t(sh.words) * size_t(n));
    AHIP_CHECK(hipStreamSynchronize(Z->stream)); // (Z's own creation may still be in flight on its stream)
    if (znnz) {
        AHIP_CHECK(hipMemcpyAsync(d->rz_idx, Z->cidx, size_t(znnz) * sizeof(int32_t), hipMemcpyDeviceToDevice, st));
        AHIP_CHECK(hipMemcpyAsync(d->rz_val, Z->cval, size_t(znnz) * vs, hipMemcpyDeviceToDevice, st));
    }
    launch_csc_block_ptr(Z->cptr, d->rz_idx, dz, nt, sh.tile_rows, d->rz_seg, st);
    DevArr<uint8_t> mbytes;
    mbytes.alloc(size_t(n) * size_t(m));
    AHIP_CHECK(hipMemcpyAsync(mbytes, mask, size_t(n) * size_t(m), hipMemcpyHostToDevice, st));
    launch_relu_sparse_pack(mbytes, n, m, d->rbits, st);
    csc_build_from_counts(
        d, md, P, nt,
        [&](int32_t* ccnt, int64_t* rcnt) { DTYPE_DISPATCH(d, launch_relu_sparse_count<T>(d->relu_csc_view<T>(), Z->rptr, ccnt, rcnt, st)) },
        [&](const int64_t* cpos) {
            DTYPE_DISPATCH(d, launch_relu_sparse_fill<T>(d->relu_csc_view<T>(), Z->rptr, Z->rcol, static_cast<const T*>(Z->rval), cpos, d->rptr,
                                                         d->cidx, static_cast<T*>(d->cval), d->rcol, static_cast<T*>(d->rval), st))
        },
        "convex_relu(): ", "convex_relu(): ");
    *out = g.release();
}

int adelie_hip_design_create_csc(const int64_t* indptr, const int32_t* indices, const void* values, const int64_t* row_indptr,
                                 const int32_t* row_indices, const void* row_values, int64_t n, int64_t p, int dtype, int device,
                                 adelie_hip_design** out) {
    ABI_TRY
    if (!indptr || !row_indptr || !out) throw make_core_error("null argument.");
    if (n <= 0 || p <= 0) throw make_core_error("matrix must have positive dimensions.");
    if (n >= (int64_t(1) << 31)) throw make_core_error("number of rows must fit in int32.");
    const size_t vs = dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float);
    if (const char* e = csc_validate_pair(indptr, indices, values, row_indptr, row_indices, row_values, n, p, vs)) throw make_core_error(e);
    const int64_t nnz = indptr[p];
    DesignGuard g(new_design(n, p, dtype, device));
    adelie_hip_design* d = g.get();
    csc_alloc(d, nnz, nullptr);
    hipStream_t s = d->stream;
    AHIP_CHECK(hipMemcpyAsync(d->cptr, indptr, size_t(p + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    AHIP_CHECK(hipMemcpyAsync(d->rptr, row_indptr, size_t(n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, s));
    if (nnz) {
        AHIP_CHECK(hipMemcpyAsync(d->cidx, indices, size_t(nnz) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        AHIP_CHECK(hipMemcpyAsync(d->cval, values, size_t(nnz) * vs, hipMemcpyHostToDevice, s));
        AHIP_CHECK(hipMemcpyAsync(d->rcol, row_indices, size_t(nnz) * sizeof(int32_t), hipMemcpyHostToDevice, s));
        AHIP_CHECK(hipMemcpyAsync(d->rval, row_values, size_t(nnz) * vs, hipMemcpyHostToDevice, s));
    }
    csc_finish(d);
    AHIP_CHECK(hipStreamSynchronize(s));
    *out = g.release();
    ABI_CATCH
}

// adelie.matrix.sparse(method="constraint"): the (m, d) matrix A kept sparse is the design kept sparse of the (d, m) matrix A'
// with the constraint flag.  A's compressed rows are the compressed columns of A' and A's compressed columns its compressed
// rows, so the two forms go to adelie_hip_design_create_csc as they are: a row of A is one compressed column.
int adelie_hip_design_create_constraint_csc(const int64_t* row_indptr, const int32_t* row_indices, const void* row_values,
                                            const int64_t* col_indptr, const int32_t* col_indices, const void* col_values, int64_t m,
                                            int64_t d, int dtype, int device, adelie_hip_design** out) {
    ABI_TRY
    if (!out) throw make_core_error("null argument.");
    if (m <= 0 || d <= 0) throw make_core_error("mat must be a non-empty (m, d) matrix.");
    if (m >= (int64_t(1) << 31) || d >= (int64_t(1) << 31)) throw make_core_error("sparse(): m and d must be below 2^31.");
    adelie_hip_design* g = nullptr;
    if (adelie_hip_design_create_csc(row_indptr, row_indices, row_values, col_indptr, col_indices, col_values, d, m, dtype, device, &g))
        throw make_core_error(g_last_error);
    g->constraint = 1;
    *out = g;
    ABI_CATCH
}

int adelie_hip_design_create_snp_phased_ancestry(const void* snpdat, int64_t n_bytes, int dtype, int device, adelie_hip_design** out) {
    ABI_TRY
    if (!snpdat || !out) throw make_core_error("null argument.");
    const uint8_t* buf = static_cast<const uint8_t*>(snpdat);
    PhasedDims dims;
    if (const char* e = phased_header(buf, n_bytes < 0 ? 0 : uint64_t(n_bytes), &dims)) throw make_core_error(e);
    std::vector<uint8_t> table(size_t(dims.n) * size_t(2 * dims.s));
    if (const char* e = phased_decode(buf, uint64_t(n_bytes), dims, table.data())) throw make_core_error(e);
    DesignGuard g(new_design(int64_t(dims.n), int64_t(dims.s * dims.A), dtype, device));
    phased_build(g.get(), table.data(), int64_t(dims.s), int(dims.A));
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_snp_phased_calldata(const int8_t* calldata, const int8_t* ancestries, int64_t n, int64_t s, int64_t A,
                                                 int dtype, int device, adelie_hip_design** out) {
    ABI_TRY
    if (!calldata || !ancestries || !out) throw make_core_error("null argument.");
    if (const char* e = phased_pack_dims(n, s, A)) throw make_core_error(e);
    std::vector<uint8_t> table(size_t(n) * size_t(2 * s));
    if (const char* e = phased_pack(calldata, ancestries, n, s, A, table.data())) throw make_core_error(e);
    DesignGuard g(new_design(n, s * A, dtype, device));
    phased_build(g.get(), table.data(), s, int(A));
    *out = g.release();
    ABI_CATCH
}

int adelie_hip_design_create_convex_relu_csc(adelie_hip_design* Z, const uint8_t* mask, int64_t m, int gated, adelie_hip_design** out) {
    ABI_TRY
    if (!Z || !out || (!mask && m > 0)) throw make_core_error("null argument.");
    if (!Z->is_csc() || Z->cov || Z->std_center || Z->constraint)
        throw make_core_error("convex_relu(): mat must be a resident design kept sparse without a standardized view on it.");
    if (m < 0) throw make_core_error("mask must be (n, m) where mat is (n, d).");
    set_device(Z);
    relu_csc_build(Z, mask, m, gated, out);
    ABI_CATCH
}

int adelie_hip_design_csc_download(adelie_hip_design* d, int64_t* indptr, int32_t* indices, void* values, int64_t* row_indptr,
                                   int32_t* row_indices, void* row_values) {
    ABI_TRY
    if (!d) throw make_core_error("null argument.");
    if (!d->is_csc()) throw make_core_error("csc_download() takes a design kept sparse.");
    if (d->cov && (row_indptr || row_indices || row_values))
        throw make_core_error("csc_download(): a covariance matrix kept sparse has the column-compressed form only.");
    set_device(d);
    hipStream_t s = d->stream;
    const size_t vs = d->dtype == ADELIE_HIP_F64 ? sizeof(double) : sizeof(float), nnz = size_t(d->nnz);
    auto down = [&](void* dst, const void* src, size_t bytes) {
        if (dst && bytes) AHIP_CHECK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, s));
    };
    down(indptr, d->cptr, size_t(d->p + 1) * sizeof(int64_t));
    down(indices, d->cidx, nnz * sizeof(int32_t));
    down(values, d->cval, nnz * vs);
    down(row_indptr, d->rptr, size_t(d->n + 1) * sizeof(int64_t));
    down(row_indices, d->rcol, nnz * sizeof(int32_t));
    down(row_values, d->rval, nnz * vs);
    AHIP_CHECK(hipStreamSynchronize(s));
    ABI_CATCH
}
int64_t adelie_hip_design_nnz(const adelie_hip_design* d) { return d && d->is_csc() ? d->nnz : -1; }
