// m3d_refine.cpp -- RefineModel (include/misc3d/common/ransac.h:534-549) and the exact / order-free error sums that decide
// fitness ties (ransac.h:595-596, 632-650): the ordered inlier list (compact_count_k + scan_blocks_k + compact_write_k, straight
// into the caller's page-locked buffer), GeneralFit from the fused moments, the serial-order sum on demand.
#include "m3d_driver_internal.hpp"
#include "m3d_generalfit_fp.hpp"
#include "m3d_mask_pool.hpp"

#pragma clang fp contract(off)

namespace m3d {

// The writers of a mask expansion (m3d_config.list_mask): the process' pool of m3d_mask_pool.hpp, sized by the configuration
static uint32_t mask_writers() { return MaskPool::writer_cap(config().list_mask); }

// Scratch of launch_compact (m3d_kernels.hpp): one slot per compaction workgroup
int compact_scratch(DeviceCtx* ctx, uint32_t nb, uint32_t** slots) {
    RESERVE(ctx->block_counts, sizeof(uint32_t) * ((size_t)nb + 1));
    *slots = ctx->block_counts.as<uint32_t>();
    return M3D_OK;
}

// EvaluateModel's (inlier_num, error) with the error summed in point order (ransac.h:632-640).
int exact_error(DeviceCtx* ctx, const CloudView& v, int kind, double thr,
                       const double* model_dev, uint64_t* count, double* error) {
    const uint32_t nb = (v.n + kCompactTile - 1) / kCompactTile;
    RESERVE(ctx->dist, sizeof(double) * (size_t)std::max<uint32_t>(v.n, 1));
    uint32_t* scratch;
    if (const int rc = compact_scratch(ctx, nb, &scratch); rc != M3D_OK) return rc;
    RESERVE(ctx->total, sizeof(uint32_t) * 4);
    RESERVE(ctx->sums, sizeof(double) * 32);
    RESERVE(ctx->h_small, 256);
    launch_compact(kind, v, model_dev, thr, 1, nullptr, nullptr, ctx->dist.as<double>(), nullptr,
                   nullptr, nullptr, nullptr, 0, scratch,
                   ctx->total.as<uint32_t>(), ctx->stream);
    launch_serial_sum(ctx->dist.as<double>(), ctx->total.as<uint32_t>(), ctx->sums.as<double>() + 16,
                      ctx->stream);
    uint8_t* h = ctx->h_small.as<uint8_t>();
    HIPCHK(hipMemcpyAsync(h, ctx->total.p, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipMemcpyAsync(h + 8, ctx->sums.as<double>() + 16, sizeof(double), hipMemcpyDeviceToHost,
                          ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    uint32_t c32;
    std::memcpy(&c32, h, 4);
    std::memcpy(error, h + 8, 8);
    *count = c32;
    return M3D_OK;
}

// Order-free sums of the inlier distances (tree) + counts of the trial model and, when its sum is not known yet, of the
// incumbent (model_b != null): enough to decide most ties (see the tie rule in run_ransac).  ONE pass over the cloud for
// both, the results stored into pinned memory by the kernel's last workgroup: one launch and one wait per tie.
int approx_error_pair(DeviceCtx* ctx, const CloudView& v, int kind, double thr, const double* model_a,
                             const double* model_b, uint64_t* count_a, double* error_a, uint64_t* count_b, double* error_b) {
    const bool fresh = ctx->tie_scratch.cap == 0;
    RESERVE(ctx->tie_scratch, sizeof(double) * (kErrorSumScratchDoubles + 2));
    RESERVE(ctx->h_tie, 64);
    uint32_t* ticket = reinterpret_cast<uint32_t*>(ctx->tie_scratch.as<double>() + kErrorSumScratchDoubles);
    if (fresh) HIPCHK(hipMemsetAsync(ticket, 0, sizeof(uint32_t), ctx->stream));
    double* h = ctx->h_tie.as<double>();
    launch_error_sum(kind, v, model_a, model_b, thr, ctx->tie_scratch.as<double>(), ticket, h, ctx->stream);
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    *count_a = (uint64_t)h[0];
    *error_a = h[1];
    if (model_b) {
        *count_b = (uint64_t)h[2];
        *error_b = h[3];
    }
    return M3D_OK;
}
int approx_error(DeviceCtx* ctx, const CloudView& v, int kind, double thr,
                        const double* model_dev, uint64_t* count, double* error) {
    return approx_error_pair(ctx, v, kind, thr, model_dev, nullptr, count, error, nullptr, nullptr);
}

// (GeneralFit's closed forms -- moments_about_mean, plane_from_moments, sphere_from_moments: m3d_generalfit_fp.hpp)

// First stage of RefineModel: the ordered inlier list of `model_dev` (+ the model record to the pinned `lazy_in`).
// total_host (pinned) receives the inlier count; *out describes what was queued.  Separate from refine() so that a
// probability-1 fit can queue it on the device's own prediction of the winner right behind the last scoring launch (run_ransac).
// fused: the model record carries the provisional centre of GeneralFit's sums (a record written by minimal_fit_k), so
// the compaction's counting pass accumulates the moments as well and no pass over the inlier list follows.
// idx_host: the caller's page-locked index list; the compaction writes it directly (the 8 bytes per inlier cross the
// host link while the kernel runs instead of in a copy command the host issues after it has woken up).
// where the compaction puts the ordered inlier list on the device (FitCaller::idx_dev)
static uint64_t* idx_dev(DeviceCtx* ctx, const FitCaller* fc) { return fc && fc->idx_dev ? fc->idx_dev : ctx->idx.as<uint64_t>(); }

int issue_refine_compaction(DeviceCtx* ctx, const CloudView& flag_view, const uint32_t* orig_dev, int kind, double thr,
                            const double* model_dev, const double* lazy_in, void* total_host, const FitCaller* fc,
                            Compaction* out, bool fused, uint64_t* idx_host, const PartitionOut* part, bool allow_mask) {
    const uint32_t n = flag_view.n;
    const uint32_t nb = (n + kCompactTile - 1) / kCompactTile;
    RESERVE(ctx->idx, sizeof(uint64_t) * (size_t)std::max<uint32_t>(n, 1));
    uint32_t* scratch;
    if (const int rc = compact_scratch(ctx, nb, &scratch); rc != M3D_OK) return rc;
    RESERVE(ctx->total, sizeof(uint32_t) * 4);
    fused = fused && kind != M3D_CYLINDER;
    if (fused) {
        RESERVE(ctx->moment_partial, sizeof(double) * 16 * (size_t)std::max<uint32_t>(nb, 1));
        RESERVE(ctx->h_moments, sizeof(double) * 2 * kFusedMomentDoubles);
    }
    // the list as a bit mask: the list has no consumer on the device (creation-order view, no partition, no device
    // destination) and refine() is the one to expand it (not a deferred RefineModel, which never waits)
    const bool early = config().mask_early != 0;   // the tail announces the mask before it folds the moments (h_sync word 2)
    const bool mask = allow_mask && fused && idx_host && nb && !orig_dev && !part && !(fc && (fc->idx_dev || fc->defer_refine)) &&
                      config().list_mask != 0;
    if (mask) {
        RESERVE(ctx->h_mask, sizeof(uint64_t) * kMaskTileWords * (size_t)nb);
        RESERVE(ctx->h_tile_counts, sizeof(uint32_t) * (size_t)nb);
        if (!ctx->h_sync.p) {
            RESERVE(ctx->h_sync, 64);
            std::memset(ctx->h_sync.p, 0, 64);
        }
        if (++ctx->mask_seq == 0) ++ctx->mask_seq;   // (never 0: the words' initial value)
        MaskPool::get().arm(mask_writers(), config().wait_spin_us);   // (the helpers wake under the device work still ahead)
    }
    launch_compact(kind, flag_view, model_dev, thr, 0, orig_dev,
                   idx_dev(ctx, fc), nullptr,
                   nullptr, nullptr, nullptr, nullptr, 0, scratch,
                   ctx->total.as<uint32_t>(), ctx->stream, const_cast<double*>(lazy_in),
                   fused ? ctx->moment_partial.as<double>() : nullptr, fused ? h_moments_at(ctx, refine_slot(fc)) : nullptr,
                   idx_host, static_cast<uint32_t*>(total_host) /* pinned: the kernel writes the total there itself */, part,
                   mask ? ctx->h_mask.as<uint64_t>() : nullptr, mask ? ctx->h_tile_counts.as<uint32_t>() : nullptr,
                   mask ? ctx->h_sync.as<uint32_t>() + 1 : nullptr, ctx->mask_seq,
                   mask && early ? ctx->h_sync.as<uint32_t>() + 2 : nullptr);
    *out = Compaction{};
    out->total = total_host;
    out->fused = fused;
    out->idx_host = idx_host;
    out->mask = mask;
    out->mask_early = mask && early;
    return M3D_OK;
}

// the list of a mask compaction into the caller's page-locked array, once the mask and the tile counts have arrived (the
// completion word, or the "mask ready" word of m3d_config.mask_early); false: the mask disagrees with `expected` or with its
// own counts (the caller redoes RefineModel with the device writing the list).  Nothing is stored outside dst[0, expected).
static bool expand_compaction_mask(DeviceCtx* ctx, uint32_t n, uint32_t expected, uint64_t* dst) {
    const uint32_t nb = (n + kCompactTile - 1) / kCompactTile;
    const uint32_t* counts = ctx->h_tile_counts.as<const uint32_t>();
    uint64_t total = 0;
    for (uint32_t t = 0; t < nb; ++t) total += counts[t];
    if (total != expected) return false;
    return MaskPool::get().expand(ctx->h_mask.as<const uint64_t>(), n, counts, dst, mask_writers());
}

// GeneralFit's closed form on the inliers' mean and centred moments: 1 and the model refined in place, or 0 and the model
// left as the best minimal model (ransac.h:204-207)
static int fit_from_moments(int kind, const double* mean, const double* moments, uint32_t ni, double* params_host) {
    double out[4];
    if (!(kind == M3D_PLANE ? plane_from_moments(mean, moments, out) : sphere_from_moments(mean, moments, (double)ni, out))) return 0;
    std::memcpy(params_host, out, sizeof(out));
    return 1;
}

// RefineModel in the order that relies on no expected count: the compaction `cp` (empty: one is queued here, the device
// writing the list, no moments, no mask), a wait for its total, the GeneralFit sums over the list, a second wait.  What
// refine() does without a usable expectation -- and how it redoes a RefineModel whose expectation, or whose mask, failed.
static int refine_in_order(DeviceCtx* ctx, const CloudView& flag_view, const CloudView& gather_view, const uint32_t* orig_dev,
                           int kind, double thr, const double* model_dev, double* params_host, size_t* inliers, size_t* n_inliers,
                           int* general_fit_ok, Compaction cp, const FitCaller* fc, bool hook_due, const double* lazy_in) {
    if (!cp.total) {
        const PartitionOut* part = fc && fc->partition_hook && orig_dev ? (*fc->partition_hook)(-1) : nullptr;
        const int rc = issue_refine_compaction(ctx, flag_view, orig_dev, kind, thr, model_dev, lazy_in, ctx->h_small.p, fc, &cp,
                                               /*fused=*/false, nullptr, part, /*allow_mask=*/false);
        if (rc != M3D_OK) return rc;
    }
    const bool idx_on_host = inliers && cp.idx_host == reinterpret_cast<uint64_t*>(inliers);
    HIPCHK(hipGetLastError());
    if (hook_due && fc && fc->before_refine_wait) {
        const int hr = (*fc->before_refine_wait)(-1);
        if (hr != M3D_OK) return hr;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (lazy_in) std::memcpy(params_host, lazy_in, sizeof(double) * kModelStride);
    uint32_t ni;
    std::memcpy(&ni, cp.total, 4);
    *n_inliers = ni;
    *general_fit_ok = 1;
    const bool need_fit = kind != M3D_CYLINDER;  // cylinder GeneralFit is a no-op, ransac.h:427-433
    const uint32_t min_pts = kind == M3D_PLANE ? 3 : 4;
    if (need_fit) {
        if (ni < min_pts) {
            *general_fit_ok = 0;  // MinimalCheck, ransac.h:166-169, 298-301
        } else {
            launch_general_fit_sums(gather_view, idx_dev(ctx, fc), ni, ctx->sum_partial.as<double>(),
                                    ctx->h_sums.as<double>(), ctx->stream);
        }
    }
    if (inliers && ni && !idx_on_host)
        HIPCHK(hipMemcpyAsync(inliers, (void*)idx_dev(ctx, fc), sizeof(uint64_t) * (size_t)ni,
                              hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipGetLastError());
    HIPCHK(hipStreamSynchronize(ctx->stream));
    if (need_fit && *general_fit_ok) {
        double sums[14];
        general_fit_sums_finish(ctx->h_sums.as<double>(), sums);
        const double mean[3] = {sums[0] / (double)ni, sums[1] / (double)ni, sums[2] / (double)ni};
        *general_fit_ok = fit_from_moments(kind, mean, sums + 4, ni, params_host);
    }
    return M3D_OK;
}

// RefineModel, ransac.h:534-549.  flag_view: cloud the distances are evaluated on; gather_view +
// orig: when the flags are computed on a compacted cloud (segmentation) the inlier list holds
// ORIGINAL indices and the GeneralFit sums gather from the original cloud (same values, same order).
// expected_ni >= 0: the inlier count is already known from the scoring pass (the usual case).  Then nothing
// has to wait for the compaction's own total: the GeneralFit sums run on the main stream while the index list
// travels to the host on the copy stream, and the total is only CHECKED at the end (a mismatch falls back to
// the synchronous order; the callers treat it as an internal error anyway).
int refine(DeviceCtx* ctx, const CloudView& flag_view, const CloudView& gather_view, const uint32_t* orig_dev, int kind, double thr,
           const double* model_dev, double* params_host, size_t* inliers, size_t* n_inliers, int* general_fit_ok, int64_t expected_ni,
           const Compaction& queued, const FitCaller* fc, bool hook_due, const double* lazy_in, bool fused) {
    const uint32_t n = flag_view.n;
    fused = fused && lazy_in != nullptr;
    RESERVE(ctx->sums, sizeof(double) * 32);
    RESERVE(ctx->sum_partial, sizeof(double) * kSumPartialDoubles);
    RESERVE(ctx->h_sums, sizeof(double) * kGeneralFitHostDoubles);
    RESERVE(ctx->h_small, 256);
    Compaction cp = queued;
    if (!cp.total) {
        uint64_t* idx_host = inliers && fused && !(fc && fc->idx_dev) &&
                                     is_library_pinned(inliers, sizeof(uint64_t) * (size_t)std::max<uint32_t>(n, 1))
                                 ? reinterpret_cast<uint64_t*>(inliers) : nullptr;
        const PartitionOut* part = fc && fc->partition_hook && orig_dev ? (*fc->partition_hook)(expected_ni) : nullptr;
        const int rc = issue_refine_compaction(ctx, flag_view, orig_dev, kind, thr, model_dev, lazy_in, ctx->h_small.p, fc, &cp,
                                               fused, idx_host, part, /*allow_mask=*/expected_ni >= 0);
        if (rc != M3D_OK) return rc;
    }
    const bool have_moments = fused && cp.fused;
    const bool idx_on_host = inliers && cp.idx_host == reinterpret_cast<uint64_t*>(inliers);
    const bool expected = expected_ni >= 0 && (uint64_t)expected_ni <= n;
    // a mask compaction queued ahead (run_ransac) serves only the path below that expands it: anything else -- no expected
    // count, another destination -- is redone with the device writing the list (the queued launches drain unread)
    if (cp.mask && !(idx_on_host && expected))
        return refine_in_order(ctx, flag_view, gather_view, orig_dev, kind, thr, model_dev, params_host, inliers, n_inliers,
                               general_fit_ok, Compaction{}, fc, hook_due, lazy_in);
    if (!expected)
        return refine_in_order(ctx, flag_view, gather_view, orig_dev, kind, thr, model_dev, params_host, inliers, n_inliers,
                               general_fit_ok, cp, fc, hook_due, lazy_in);
    const uint32_t ni_e = (uint32_t)expected_ni;
    const bool need_fit_e = kind != M3D_CYLINDER && ni_e >= (kind == M3D_PLANE ? 3u : 4u);
    if (!cp.ev_recorded) HIPCHK(hipEventRecord(ctx->ev_compact, ctx->stream));
    // page-locked destination (m3d_host_alloc): the index list leaves NOW, on the copy stream, under the sums
    // (or has been written by the compaction itself: idx_on_host)
    const bool early_copy = !idx_on_host && inliers && ni_e && is_library_pinned(inliers, sizeof(uint64_t) * (size_t)ni_e);
    if (early_copy) {
        HIPCHK(hipStreamWaitEvent(copy_stream_of(ctx), ctx->ev_compact, 0));
        HIPCHK(hipMemcpyAsync(inliers, (void*)idx_dev(ctx, fc),
                              sizeof(uint64_t) * (size_t)ni_e, hipMemcpyDeviceToHost, copy_stream_of(ctx)));
    }
    if (need_fit_e && !have_moments) {
        launch_general_fit_sums(gather_view, idx_dev(ctx, fc), ni_e, ctx->sum_partial.as<double>(),
                                ctx->h_sums.as<double>(), ctx->stream);
    }
    // work the caller wants queued behind these kernels before the host waits (segmentation: the removal of
    // these very inliers), so that ONE wait covers both
    const bool hooked = hook_due && fc && fc->before_refine_wait;
    if (hooked) {
        const int hr = (*fc->before_refine_wait)(expected_ni);
        if (hr != M3D_OK) return hr;
    }
    // last: a copy into the caller's (pageable) buffer keeps the host busy until it is done
    if (inliers && ni_e && !early_copy && !idx_on_host) {
        HIPCHK(hipStreamWaitEvent(copy_stream_of(ctx), ctx->ev_compact, 0));
        HIPCHK(hipMemcpyAsync(inliers, (void*)idx_dev(ctx, fc),
                              sizeof(uint64_t) * (size_t)ni_e, hipMemcpyDeviceToHost, copy_stream_of(ctx)));
    }
    HIPCHK(hipGetLastError());
    // everything RefineModel reads is complete at ev_compact when the moments rode on the compaction (or no fit is
    // due): what the hook queued behind it (segmentation: the removal of these inliers, tens of microseconds of
    // kernels) is not waited for -- the caller goes on preparing the next round under it
    bool expanded = false, expand_ok = true;   // (mask_early: the list is written before the completion word is waited for)
    if (hooked && (have_moments || !need_fit_e)) {
        HIPCHK(hipEventSynchronize(ctx->ev_compact));
    } else if (cp.mask && !hooked) {
        // nothing of RefineModel follows the compaction: its last launch stored the completion word itself
        if (cp.mask_early && ni_e) {
            // ... and the "mask ready" word first: the mask and the tile counts came with the launch before it, and the list
            // needs nothing else -- it is written while that launch folds the moments; the total is checked further down
            // (here: the sum of the tile counts against the expectation, before the first store)
            const int erc = word_wait_spin(ctx, ctx->h_sync.as<uint32_t>() + 2, ctx->mask_seq);
            if (erc != M3D_OK) return erc;
            expand_ok = expand_compaction_mask(ctx, n, ni_e, reinterpret_cast<uint64_t*>(inliers));
            expanded = true;
        }
        const int wrc = word_wait_spin(ctx, ctx->h_sync.as<uint32_t>() + 1, ctx->mask_seq);
        if (wrc != M3D_OK) return wrc;
    } else {
        const int wrc = stream_wait_spin(ctx);
        if (wrc != M3D_OK) return wrc;
    }
    // (the copy stream is waited for when THIS call put the list on it -- and not even then when the caller collects
    // its lists at the end: FitCaller::defer_copy_sync)
    const bool list_on_copy_stream = inliers && ni_e && !idx_on_host;
    if (list_on_copy_stream && !(fc && fc->defer_copy_sync && fc->idx_dev)) HIPCHK(hipStreamSynchronize(copy_stream_of(ctx)));
    if (lazy_in) std::memcpy(params_host, lazy_in, sizeof(double) * kModelStride);
    uint32_t ni_chk;
    std::memcpy(&ni_chk, cp.total, 4);
    // (a mask compaction: the host writes the list now -- the total it checks is the sum of the tile counts)
    if (ni_chk != ni_e ||   // should not happen: redo in the order that does not rely on the expectation (the hook has run)
        (cp.mask && ni_e && !(expanded ? expand_ok : expand_compaction_mask(ctx, n, ni_e, reinterpret_cast<uint64_t*>(inliers)))))
        return refine_in_order(ctx, flag_view, gather_view, orig_dev, kind, thr, model_dev, params_host, inliers, n_inliers,
                               general_fit_ok, Compaction{}, fc, /*hook_due=*/false, /*lazy_in=*/nullptr);
    *n_inliers = ni_e;
    *general_fit_ok = 1;
    if (kind != M3D_CYLINDER && !need_fit_e) {
        *general_fit_ok = 0;  // MinimalCheck, ransac.h:166-169, 298-301
    } else if (kind != M3D_CYLINDER) {
        double sums[14];
        double mean[3];
        if (have_moments) {
            // raw moments about the record's provisional centre (slots 4..6: a point among the samples) -> mean +
            // centred moments (m3d_generalfit_fp.hpp)
            const double* rec = lazy_in;
            const double c0[3] = {rec[4], rec[5], rec[6]};
            moments_about_mean(h_moments_at(ctx, refine_slot(fc)), c0, (double)ni_e, mean, sums + 4);
        } else {
            general_fit_sums_finish(ctx->h_sums.as<double>(), sums);
            for (int k = 0; k < 3; ++k) mean[k] = sums[k] / (double)ni_e;
        }
        *general_fit_ok = fit_from_moments(kind, mean, sums + 4, ni_e, params_host);
    }
    return M3D_OK;
}

}  // namespace m3d

using namespace m3d;

extern "C" {

int m3d_cloud_exact_error(m3d_cloud* c, int kind, double threshold, const double* model,
                          uint64_t* count, double* error) {
    if (!c || kind < 0 || kind > 2 || !model || !count || !error)
        return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    DeviceCtx* ctx = c->ctx;
    CtxLock lock(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    RESERVE(ctx->small, 256);
    double tmp[kModelStride] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(tmp, model, sizeof(double) * num_params(kind));
    HIPCHK(hipMemcpyAsync(ctx->small.p, tmp, sizeof(tmp), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));  // tmp is a stack buffer
    return exact_error(ctx, c->view(), kind, threshold, ctx->small.as<double>(), count, error);
}

int m3d_cloud_refine_expect(m3d_cloud* c, int kind, double threshold, double* params, int64_t expected_inliers,
                            size_t* inliers, size_t* n_inliers) {
    if (!c || kind < 0 || kind > 2 || !params || !n_inliers)
        return fail(M3D_ERR_INVALID_ARG, "invalid argument");
    DeviceCtx* ctx = c->ctx;
    CtxLock lock(ctx);
    HIPCHK(hipSetDevice(ctx->device));
    RESERVE(ctx->small, 256);
    RESERVE(ctx->h_small, 256);
    double tmp[kModelStride] = {0, 0, 0, 0, 0, 0, 0, 0};
    std::memcpy(tmp, params, sizeof(double) * num_params(kind));
    // staged through pinned memory (bytes 192.. of h_small; refine() uses the first 128): no host wait before the launches
    std::memcpy(ctx->h_small.as<uint8_t>() + 192, tmp, sizeof(tmp));
    HIPCHK(hipMemcpyAsync(ctx->small.p, ctx->h_small.as<uint8_t>() + 192, sizeof(tmp), hipMemcpyHostToDevice, ctx->stream));
    int gf = 1;
    const CloudView v = c->view();
    const int rc = refine(ctx, v, c->base_view(), c->orig(), kind, threshold, ctx->small.as<double>(), tmp, inliers,
                          n_inliers, &gf, expected_inliers, Compaction{}, nullptr);
    if (rc != M3D_OK) return rc;
    std::memcpy(params, tmp, sizeof(double) * num_params(kind));
    return gf ? M3D_OK : M3D_FALSE;
}
int m3d_cloud_refine(m3d_cloud* c, int kind, double threshold, double* params, size_t* inliers,
                     size_t* n_inliers) {
    return m3d_cloud_refine_expect(c, kind, threshold, params, -1, inliers, n_inliers);
}


}  // extern "C"
