// sm_delta_host.hpp - host paths of the delta operators: TIES, DARE, Breadcrumbs, the geometric and Karcher-mean
// merges, SCE, DELLA, Consensus, the pairwise fusion, PCB, TSV, WIDEN, CABS, Iso-C, the task-vector statistics, the low-rank extraction, the delta pack and EMR-Merging (sm_delta.hpp
// and the operators' headers; the functions are stated in shardmerge_hip.h; arguments checked in sm_capi.inc).
// DeltaHost<B> is a member of Pipeline<B> (sm_pipeline.hpp): it launches on the pipeline's backend and stream, reports
// through its error string and owns the one workspace buffer the operators share - they never run at once.
// The passes that several operators launch are written once, ahead of the operators.
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/shardmerge_hip.h"
#include "sm_ties.hpp"
#include "sm_dare.hpp"
#include "sm_breadcrumbs.hpp"
#include "sm_geo.hpp"
#include "sm_sphere.hpp"
#include "sm_sce.hpp"
#include "sm_della.hpp"
#include "sm_consensus.hpp"
#include "sm_stats.hpp"
#include "sm_extract.hpp"
#include "sm_fusion.hpp"
#include "sm_pcb.hpp"
#include "sm_tsv.hpp"
#include "sm_widen.hpp"
#include "sm_cabs.hpp"
#include "sm_iso.hpp"
#include "sm_dpack.hpp"
#include "sm_emr.hpp"
#include "sm_emr_fused.hpp"

namespace smhip {

// ---- what every host path uses, the spectral pipeline's included -------------------------------
struct Buffer {
    void* p = nullptr;
    size_t cap = 0;
};
inline size_t round_up(size_t v, size_t m) { return (v + m - 1) / m * m; }
// grows b to at least `bytes` (its contents are lost); the stream drains before the old block is freed.  false: no memory
template <class B>
bool grow_buffer(B& be, void* stream, Buffer& b, size_t bytes) {
    if (b.cap >= bytes) return true;
    if (b.p) { be.sync(stream); be.free(b.p); b.p = nullptr; b.cap = 0; }
    b.p = be.alloc(bytes);
    if (!b.p) return false;
    b.cap = bytes;
    return true;
}
// chunks per thread such that a streaming kernel runs about `waves` work-groups per
// CU in total: the per-work-group fixed costs (LDS histogram zero/flush, staging,
// block reductions, atomics) are paid once per resident work-group, not per 8K elements
inline int pick_chunks(size_t units, int block, int min_chunks, int wgs_per_cu = 5) {
    const size_t target = (size_t)256 * wgs_per_cu;
    size_t c = (units + (size_t)block * target - 1) / ((size_t)block * target);
    if (c < (size_t)min_chunks) c = min_chunks;
    if (c > 4096) c = 4096;
    return (int)c;
}
inline int stream_grid(size_t units, int block, int chunks) {
    const size_t per = (size_t)block * chunks;
    size_t g = (units + per - 1) / per;
    return (int)std::max<size_t>(g, 1);
}
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }

template <class B>
class DeltaHost {
  public:
    B& be;
    std::string& err;
    void*& stream;
    size_t della_slab_rows = 0;               // test hook "della_slab_rows": rows per slab (0: at most 2^26 elements per finetune)
    unsigned long long eig_host_us = 0;       // debug query "eig_host_us": host time in xl_sym_eig since the context was created

    DeltaHost(B& be_, std::string& err_, void*& stream_) : be(be_), err(err_), stream(stream_) {}
    ~DeltaHost() { if (ws_.p) be.free(ws_.p); }
    DeltaHost(const DeltaHost&) = delete;

    int fail(int code, const std::string& msg) { err = msg; return code; }
    size_t workspace_bytes() const { return ws_.cap; }

    // ---- the shared passes.  The descriptors share their leading fields and the *MergeParams their common ones, so what the
    // host paths share is written once, as templates. ----
    static unsigned long long delta_k_keep(double density, size_t n) {
        return density == 1.0 ? (unsigned long long)n : (unsigned long long)std::floor(density * (double)n);
    }
    // the k inputs padded with finetune 0, whether they share one base, and their alignment on top of `al`, that of the
    // call's other tensors.  base == nullptr (weight space): the vectors are the finetunes themselves, no base is read
    static void ties_inputs(TiesInputs& in, int k, int dtype, size_t n, const void* const* ft, const void* const* base, bool al) {
        in.k = k; in.dtype = dtype; in.n = n;
        bool shared = true;
        for (int i = 0; i < TIES_MAX_MODELS; ++i) {
            in.ft[i] = ft[i < k ? i : 0]; in.base[i] = base ? base[i < k ? i : 0] : nullptr;
            al = al && aligned16(in.ft[i]) && aligned16(in.base[i]);
            shared = shared && in.base[i] == in.base[0];
        }
        in.aligned = al ? 1 : 0; in.shared_base = shared ? 1 : 0;
    }
    // what every merge descriptor has: the inputs, the outputs (in weight space base_out need not be aligned), add-back, chunks
    template <class Desc, class Params>
    void delta_inputs(const Desc& d, void* out, float* delta_out, bool weight_space, Params& m) {
        ties_inputs(m.in, d.k, d.in_dtype, d.n, d.finetune, weight_space ? (const void* const*)nullptr : d.base,
                    aligned16(out) && aligned16(delta_out) && (weight_space || aligned16(d.base_out)));
        m.base_out = d.base_out; m.base_out_dtype = d.base_out_dtype;
        m.out_is_base0 = (!weight_space && m.in.shared_base && d.base_out == m.in.base[0] && d.base_out_dtype == d.in_dtype) ? 1 : 0;
        m.out = out; m.delta_out = delta_out;
        m.chunks = pick_chunks((d.n + 7) / 8, 256, 2, 8);
    }
    // ... and what the descriptors of the election operators add: the weights, lambda, normalize
    template <class Desc, class MergeParams>
    void delta_merge_params(const Desc& d, void* out, float* delta_out, MergeParams& m) {
        delta_inputs(d, out, delta_out, false, m);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.alpha[i] = (float)d.alpha[i < d.k ? i : 0];
        m.lambda = (float)d.lambda; m.normalize = d.normalize ? 1 : 0;
    }
    // a non-finite vector fails the call: the message names the entry point, what the vectors are, and the finetunes whose
    // bit is set in a fetched flag word
    int delta_nonfinite(const char* op, const char* vectors, int k, uint32_t flags) {
        std::string which;
        for (int i = 0; i < k; ++i)
            if (flags & (1u << i)) which += (which.empty() ? "" : ", ") + std::to_string(i);
        return fail(SMHIP_ERR_NONFINITE, std::string(op) + ": NaN or Inf in " + vectors + " of finetune " + which);
    }
    // the call's one synchronisation: fetch the readback and fail on a non-finite delta (flags[0]: one bit per finetune)
    template <class Readback>
    int delta_readback(const char* op, int k, const Readback* rb, Readback& host) {
        be.d2h(&host, rb, sizeof host, stream);
        if (!be.ok()) { host = Readback{}; return SMHIP_OK; }   // (reported by the caller as SMHIP_ERR_HIP; the report stays zero)
        if (!host.flags[0]) return SMHIP_OK;
        return delta_nonfinite(op, "finetune - base", k, host.flags[0]);
    }
    // the workspace of an operator without a select: `total` bytes of which the Head at their start is zeroed
    template <class Head>
    int plain_workspace(Head*& head, size_t total = sizeof(Head)) {
        if (!grow_buffer(be, stream, ws_, total)) return fail(SMHIP_ERR_NOMEM, "workspace allocation failed");
        be.memset(ws_.p, 0, sizeof(Head), stream);
        head = (Head*)ws_.p;
        return SMHIP_OK;
    }
    // the workspace of a radix select: the three levels' histograms [3][streams][HIST1_BINS] | Tail, zeroed; then, from
    // the next multiple of 256 bytes (*off_more) on, `more` bytes that are not
    static size_t select_hist_level(int streams) { return (size_t)streams * HIST1_BINS * sizeof(unsigned long long); }
    template <class Tail>
    int select_workspace(int streams, Tail*& tail, size_t more = 0, size_t* off_more = nullptr) {
        const size_t off_tail = 3 * select_hist_level(streams), zeroed = off_tail + sizeof(Tail), off = round_up(zeroed, 256);
        if (!grow_buffer(be, stream, ws_, more ? off + more : zeroed)) return fail(SMHIP_ERR_NOMEM, "workspace allocation failed");
        be.memset(ws_.p, 0, zeroed, stream);
        tail = (Tail*)((char*)ws_.p + off_tail);
        if (off_more) *off_more = off;
        return SMHIP_OK;
    }
    char* ws_at(size_t off) { return (char*)ws_.p + off; }
    // the three levels of a radix select: launch_hist(level, hist) fills the level's histograms, then one select launch
    // of `grid` work-groups.  The caller has filled s but for the level and hist of lv, which is s or its part with them.
    template <class KSelect, class SelectParams, class Levels, class LaunchHist>
    void select_levels(int streams, int grid, SelectParams& s, Levels& lv, size_t select_lds, LaunchHist&& launch_hist) {
        for (int level = 1; level <= 3; ++level) {
            unsigned long long* hist = (unsigned long long*)ws_at((size_t)(level - 1) * select_hist_level(streams));
            launch_hist(level, hist);
            lv.level = level; lv.hist = hist;
            be.template launch<KSelect>(grid, TIES_SELECT_THREADS, select_lds, s, stream);
        }
    }
    // the grid of a *_hist launch over the octets of h.in, h.chunks per thread
    template <class HistParams>
    static int hist_grid(HistParams& h) {
        const size_t noct = (h.in.n + 7) / 8;
        h.chunks = pick_chunks(noct, 256, 4, 5);
        return stream_grid(noct, 256, h.chunks);
    }
    // ... with a select work-group per finetune: hist launches in groups of TIES_GROUP finetunes.  The caller has filled h
    // but for level, hist, first, count and chunks; hist_words(level): LDS words per finetune; level1_only: a select that
    // keeps nothing has thresholds of +inf whatever the data, and only level 1, which finds the non-finite deltas, runs
    template <class KHist, class KSelect, class HistParams, class SelectParams, class HistWords>
    void select_levels_per_finetune(int streams, HistParams& h, SelectParams& s, size_t select_lds, HistWords&& hist_words,
                                    bool level1_only) {
        const int k = h.in.k, hgrid = hist_grid(h);
        select_levels<KSelect>(streams, k, s, s, select_lds, [&](int level, unsigned long long* hist) {
            h.level = level; h.hist = hist;
            for (int first = 0; first < k && (level == 1 || !level1_only); first += TIES_GROUP) {
                h.first = first; h.count = std::min(TIES_GROUP, k - first);
                be.template launch<KHist>(hgrid, 256, (LDS_SCRATCH_FLOATS + (size_t)h.count * hist_words(level)) * 4, h, stream);
            }
        });
    }
    // the thresholds of TIES, one rank per finetune (levels 2 and 3 need only the low bins in LDS), into a select_workspace
    // tail of TiesWork's shape: state, rb.threshold, rb.kept, rb.flags
    template <class Work>
    void ties_thresholds(const TiesInputs& in, unsigned long long k_keep, Work* w) {
        TiesHistParams h;
        h.in = in; h.state = w->state; h.flags = w->rb.flags;
        TiesSelectParams s;
        s.k_keep = k_keep; s.state = w->state; s.threshold = w->rb.threshold; s.kept = w->rb.kept;
        select_levels_per_finetune<KTiesHist, KTiesSelect>(TIES_MAX_MODELS, h, s, TIES_SELECT_LDS,
                                                           [](int level) { return radix_bins(level); }, k_keep == 0);
    }
    // The ordered fp64 fold (k_geo_fold, sm_geo.hpp) of part[nseg][np] under the tag K: into out[np], or with row > 0 as
    // rows of `row` values `pitch` apart
    template <class K>
    void fold_pass(int np, size_t nseg, const double* part, double* out, int row = 0, int pitch = 0) {
        GeoFoldParams f;
        f.np = np; f.row = row ? row : np; f.pitch = row ? pitch : np; f.nseg = nseg; f.part = part; f.out = out;
        be.template launch<K>(1, 256, LDS_SCRATCH_FLOATS * 4, f, stream);
    }
    // The ordered fp64 Gram pass (sm_geo.hpp) over nseg segments of seg_len elements: a work-group per segment and tile of
    // pairs, the segments' partials into part, a bit per non-finite vector into flags[0]; G: folded over the segments into
    // it, or nullptr.  gram_grid is the bound on that grid, for the caller to check before its workspace grows.
    int gram_grid(const char* op, int k, size_t nseg) {
        if (nseg * (size_t)geo_tiles(k) > (size_t)0x7fffffff) return fail(SMHIP_ERR_ARG, std::string(op) + ": tensor too large");
        return SMHIP_OK;
    }
    void gram_pass(const TiesInputs& in, bool weight_space, size_t seg_len, size_t nseg, double* part, uint32_t* flags, double* G) {
        GeoGramParams g;
        g.in = in; g.weight_space = weight_space ? 1 : 0;
        g.seg_len = seg_len; g.nseg = nseg; g.seg_vec = (in.aligned && seg_len % 8 == 0) ? 1 : 0;
        g.part = part; g.flags = flags;
        const int grid = (int)(nseg * (size_t)geo_tiles(in.k));
        if (in.k <= GEO_TILE) be.template launch<KGeoGram>(grid, GEO_THREADS, geo_gram_lds_floats() * 4, g, stream);
        else be.template launch<KGeoGramTiled>(grid, GEO_THREADS, geo_gram_lds_floats() * 4, g, stream);
        if (G) fold_pass<KGeoFold>(geo_pairs(in.k), nseg, part, G);
    }

    // ---- TIES merge ----
    struct TiesReadback { float threshold[TIES_MAX_MODELS]; unsigned long long kept[TIES_MAX_MODELS]; uint32_t flags[2]; };
    struct TiesWork { RadixState state[TIES_MAX_MODELS]; TiesReadback rb; };
    int ties_merge(const smhip_ties_desc& d, void* out, float* delta_out, smhip_ties_report* rep) {
        const int k = d.k;
        const unsigned long long k_keep = delta_k_keep(d.density, d.n);
        if (rep) {
            rep->k_keep = k_keep;
            for (int i = 0; i < SMHIP_MAX_MODELS; ++i) { rep->threshold[i] = 0.f; rep->kept[i] = 0; }
        }
        if (d.n == 0) {                                  // k_keep == 0: the threshold is +inf by definition
            if (rep) for (int i = 0; i < k; ++i) rep->threshold[i] = INFINITY;
            return SMHIP_OK;
        }
        TiesWork* w;
        int rc;
        if ((rc = select_workspace(TIES_MAX_MODELS, w))) return rc;

        TiesMergeParams m;
        delta_merge_params(d, out, delta_out, m);
        m.threshold = w->rb.threshold;
        ties_thresholds(m.in, k_keep, w);
        be.template launch<KTiesMerge>(stream_grid((d.n + 7) / 8, 256, m.chunks), 256, LDS_SCRATCH_FLOATS * 4, m, stream);

        TiesReadback host;
        if ((rc = delta_readback("ties_merge", k, &w->rb, host))) return rc;
        if (rep)
            for (int i = 0; i < k; ++i) { rep->threshold[i] = host.threshold[i]; rep->kept[i] = host.kept[i]; }
        return SMHIP_OK;
    }

    // ---- DARE merge: no select, one kernel; the workspace is DareReadback.  dare_pass is the call for any descriptor with
    // DARE's fields (smhip_dare_desc; smhip_della_desc with a uniform threshold); op names the entry point in the error text ----
    struct DareReadback { unsigned long long kept[TIES_MAX_MODELS]; uint32_t flags[2]; };
    static uint32_t dare_threshold(double density) {
        return density == 1.0 ? DARE_T_ONE : (uint32_t)std::floor(density * 65536.0);
    }
    template <class Desc, class MergeParams>
    void dare_fields(const Desc& d, DareReadback* rb, MergeParams& m) {
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.stream_id[i] = d.stream_id[i < d.k ? i : 0];
        m.key = d.key; m.sign_election = d.sign_election ? 1 : 0;
        m.kept = rb->kept; m.flags = rb->flags;
    }
    int dare_readback(const char* op, int k, const DareReadback* rb, uint64_t* kept) {
        DareReadback host;
        int rc;
        if ((rc = delta_readback(op, k, rb, host))) return rc;
        if (kept)
            for (int i = 0; i < k; ++i) kept[i] = host.kept[i];
        return SMHIP_OK;
    }
    template <class Desc>
    int dare_pass(const char* op, const Desc& d, uint32_t T, void* out, float* delta_out, uint64_t* kept) {
        DareReadback* rb;
        int rc;
        if ((rc = plain_workspace(rb))) return rc;

        DareMergeParams m;
        delta_merge_params(d, out, delta_out, m);
        dare_fields(d, rb, m);
        m.T = T;
        m.rescale = d.rescale ? (float)(65536.0 / (double)T) : 1.f;
        be.template launch<KDareMerge>(stream_grid((d.n + 7) / 8, 256, m.chunks), 256, (LDS_SCRATCH_FLOATS + dare_lds_words(d.k, 256)) * 4, m, stream);
        return dare_readback(op, d.k, rb, kept);
    }
    int dare_merge(const smhip_dare_desc& d, void* out, float* delta_out, smhip_dare_report* rep) {
        const uint32_t T = dare_threshold(d.density);
        if (rep) {
            rep->T = T;
            for (int i = 0; i < SMHIP_MAX_MODELS; ++i) rep->kept[i] = 0;
        }
        if (d.n == 0) return SMHIP_OK;
        return dare_pass("dare_merge", d, T, out, delta_out, rep ? rep->kept : nullptr);
    }

    // ---- Breadcrumbs merge: two ranks per finetune (RadixState[k][2]), found in the same three histogram passes ----
    struct CrumbsReadback {
        float threshold_lo[TIES_MAX_MODELS], threshold_hi[TIES_MAX_MODELS];
        unsigned long long kept[TIES_MAX_MODELS], dropped_top[TIES_MAX_MODELS];
        uint32_t flags[2];
    };
    struct CrumbsWork { RadixState state[2 * TIES_MAX_MODELS]; CrumbsReadback rb; };
    int breadcrumbs_merge(const smhip_breadcrumbs_desc& d, void* out, float* delta_out, smhip_breadcrumbs_report* rep) {
        const int k = d.k;
        const unsigned long long k_keep = delta_k_keep(d.density, d.n);
        const unsigned long long n_top = std::min((unsigned long long)std::floor(d.gamma * (double)d.n), (unsigned long long)d.n - k_keep);
        if (rep) {
            rep->k_keep = k_keep; rep->n_top = n_top;
            for (int i = 0; i < SMHIP_MAX_MODELS; ++i) { rep->threshold_lo[i] = 0.f; rep->threshold_hi[i] = 0.f; rep->kept[i] = 0; rep->dropped_top[i] = 0; }
        }
        if (d.n == 0) {                                  // k_keep == 0: the thresholds are +inf by definition
            if (rep) for (int i = 0; i < k; ++i) { rep->threshold_lo[i] = INFINITY; rep->threshold_hi[i] = INFINITY; }
            return SMHIP_OK;
        }
        CrumbsWork* w;
        int rc;
        if ((rc = select_workspace(TIES_MAX_MODELS, w))) return rc;

        CrumbsMergeParams m;
        delta_merge_params(d, out, delta_out, m);
        m.sign_election = d.sign_election ? 1 : 0;
        m.threshold_lo = w->rb.threshold_lo; m.threshold_hi = w->rb.threshold_hi;

        CrumbsHistParams h;
        h.in = m.in; h.state = w->state; h.flags = w->rb.flags;
        CrumbsSelectParams s;
        s.k_keep = k_keep; s.rank[CRUMBS_HI] = n_top + 1; s.rank[CRUMBS_LO] = n_top + k_keep;
        s.state = w->state; s.threshold_lo = w->rb.threshold_lo; s.threshold_hi = w->rb.threshold_hi;
        s.kept = w->rb.kept; s.dropped_top = w->rb.dropped_top;
        select_levels_per_finetune<KCrumbsHist, KCrumbsSelect>(TIES_MAX_MODELS, h, s, CRUMBS_SELECT_LDS,
                                                               [](int) { return HIST1_BINS; }, k_keep == 0);
        be.template launch<KCrumbsMerge>(stream_grid((d.n + 7) / 8, 256, m.chunks), 256, LDS_SCRATCH_FLOATS * 4, m, stream);

        CrumbsReadback host;
        if ((rc = delta_readback("breadcrumbs_merge", k, &w->rb, host))) return rc;
        if (rep)
            for (int i = 0; i < k; ++i) {
                rep->threshold_lo[i] = host.threshold_lo[i]; rep->threshold_hi[i] = host.threshold_hi[i];
                rep->kept[i] = host.kept[i]; rep->dropped_top[i] = host.dropped_top[i];
            }
        return SMHIP_OK;
    }

    // ---- Geometric and Karcher-mean merges: what geo_merge and sphere_merge share.  The Gram pass, then whole tensor: its
    // fold, ONE readback, the coefficients on the host, the combine pass; row-wise: the operator's coefficient kernel over the
    // rows' Grams, the combine pass through its row-coefficient path, the readbacks at the end.
    // Workspace: GeoHead | partials or row Grams | row coefficients | the operator's row data ----
    struct GeoHead { uint32_t flags[2]; double G[TIES_MAX_MODELS * (TIES_MAX_MODELS + 1) / 2]; };
    struct GeoRun {
        GeoCombineParams m;        // the combine pass: all but its coefficients
        int cgrid;
        size_t nseg;               // segments; row-wise: the rows
        GeoHead* head;
        double* part;
        float* coef;               // row-wise: [nseg][k]
        char* rows;                // row-wise: the operator's row_bytes(nseg) bytes
    };
    template <class Desc>
    int geo_begin(const char* op, const Desc& d, void* out, float* delta_out, bool weight, size_t (*row_bytes)(size_t), GeoRun& r) {
        const int k = d.k;
        const bool rowwise = d.rowwise != 0;
        GeoCombineParams& m = r.m;
        delta_inputs(d, out, delta_out, weight, m);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.c[i] = 0.f;
        m.weight_space = weight ? 1 : 0;
        m.rowcoef = nullptr; m.C = d.n / d.rows;
        r.cgrid = stream_grid((d.n + 7) / 8, 256, m.chunks);
        const size_t seg_len = rowwise ? m.C : GEO_SEG_ELEMS;
        r.nseg = (d.n + seg_len - 1) / seg_len;
        int rc;
        if ((rc = gram_grid(op, k, r.nseg))) return rc;

        const size_t off_part = round_up(sizeof(GeoHead), 256), part_bytes = round_up(r.nseg * geo_pairs(k) * sizeof(double), 256);
        const size_t off_coef = off_part + part_bytes, coef_bytes = rowwise ? round_up(r.nseg * k * sizeof(float), 256) : 0;
        const size_t off_rows = off_coef + coef_bytes;
        if ((rc = plain_workspace(r.head, off_rows + (rowwise ? row_bytes(r.nseg) : 0)))) return rc;
        r.part = (double*)ws_at(off_part); r.coef = (float*)ws_at(off_coef); r.rows = ws_at(off_rows);
        gram_pass(m.in, weight, seg_len, r.nseg, r.part, r.head->flags, rowwise ? nullptr : r.head->G);
        return SMHIP_OK;
    }
    // fetches the head - whole tensor: the call's one synchronisation - and fails on a non-finite vector
    int geo_head(const char* op, int k, const GeoRun& r, GeoHead& host) {
        be.d2h(&host, r.head, sizeof host, stream);
        if (!be.ok() || !host.flags[0]) return SMHIP_OK;        // (a device error: reported by the caller as SMHIP_ERR_HIP)
        return delta_nonfinite(op, "the vector (finetune - base, or the finetune)", k, host.flags[0]);
    }

    // ---- Geometric merges (sm_geo.hpp; smhip_geo_merge).  Row data: t [rows] ----
    int geo_merge(const smhip_geo_desc& d, void* out, float* delta_out, smhip_geo_report* rep) {
        const int k = d.k;
        if (rep) *rep = smhip_geo_report{};
        // the scalars that need no data
        double A = 0.0;
        for (int i = 0; i < k; ++i) A = geo_dadd(A, d.alpha[i]);
        if (std::fabs(A) < 1e-8) A = 1.0;
        const double tau = (d.mode != SMHIP_GEO_MODEL_STOCK && k == 2) ? geo_ddiv(d.alpha[1], geo_dadd(d.alpha[0], d.alpha[1])) : 0.0;
        if (d.n == 0) return SMHIP_OK;

        GeoRun r;
        int rc;
        if ((rc = geo_begin("geo_merge", d, out, delta_out, d.mode == SMHIP_GEO_SLERP, [](size_t R) { return R * sizeof(double); }, r))) return rc;
        GeoCombineParams& m = r.m;
        GeoHead host;
        if (d.rowwise) {
            GeoCoefParams c;
            c.k = k; c.rows = r.nseg; c.A = A; c.G = r.part;
            for (int i = 0; i < TIES_MAX_MODELS; ++i) c.alpha[i] = d.alpha[i < k ? i : 0];
            c.coef = r.coef; c.t = (double*)r.rows;
            be.template launch<KGeoCoef>((int)((r.nseg + 255) / 256), 256, LDS_SCRATCH_FLOATS * 4, c, stream);
            m.rowcoef = c.coef;
            be.template launch<KGeoCombine>(r.cgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
            std::vector<double> t(r.nseg);
            be.d2h(t.data(), c.t, r.nseg * sizeof(double), stream);      // (the call's one synchronisation; the head follows on the drained stream)
            if ((rc = geo_head("geo_merge", k, r, host)) || !be.ok()) return rc;
            if (rep) {
                double sum = 0.0, lo = t[0], hi = t[0];
                for (double v : t) { sum = geo_dadd(sum, v); lo = std::min(lo, v); hi = std::max(hi, v); }
                rep->t_min = lo; rep->t_max = hi; rep->t_mean = geo_ddiv(sum, (double)r.nseg);
            }
            return SMHIP_OK;
        }

        if ((rc = geo_head("geo_merge", k, r, host)) || !be.ok()) return rc;
        const double* G = host.G;
        double cosv = 0.0, tv = 0.0, omega = 0.0;
        int linear = 0;
        if (d.mode == SMHIP_GEO_MODEL_STOCK) {
            tv = geo_stock_t(G, k, &cosv);
            for (int i = 0; i < k; ++i) m.c[i] = geo_stock_coef(tv, d.alpha[i], A);
        } else if (k == 1) {
            m.c[0] = 1.f; linear = 1;
        } else {
            const double n0 = geo_dsqrt(G[geo_pair_index(0, 0, 2)]), n1 = geo_dsqrt(G[geo_pair_index(1, 1, 2)]);
            cosv = geo_cos(G[geo_pair_index(0, 1, 2)], n0, n1);
            tv = tau;
            double s0, s1;
            const double one_tau = geo_dadd(1.0, -tau);
            linear = (n0 == 0.0 || n1 == 0.0 || std::fabs(cosv) > 0.9995) ? 1 : 0;
            if (linear) {
                s0 = one_tau; s1 = tau;
            } else {
                omega = std::acos(cosv);
                const double so = std::sin(omega);
                s0 = geo_ddiv(std::sin(geo_dmul(one_tau, omega)), so);
                s1 = geo_ddiv(std::sin(geo_dmul(tau, omega)), so);
            }
            if (d.mode == SMHIP_GEO_NUSLERP && !linear) {
                const double N = geo_dadd(geo_dmul(one_tau, n0), geo_dmul(tau, n1));
                m.c[0] = (float)geo_ddiv(geo_dmul(s0, N), n0);
                m.c[1] = (float)geo_ddiv(geo_dmul(s1, N), n1);
            } else {
                m.c[0] = (float)s0; m.c[1] = (float)s1;
            }
        }
        if (rep) {
            for (int i = 0; i < k; ++i)
                for (int j = i; j < k; ++j) rep->G[i][j] = rep->G[j][i] = G[geo_pair_index(i, j, k)];
            rep->cos = cosv; rep->t = tv; rep->omega = omega; rep->linear = linear;
            for (int i = 0; i < k; ++i) rep->c[i] = m.c[i];
        }
        be.template launch<KGeoCombine>(r.cgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
        return SMHIP_OK;
    }

    // ---- Karcher-mean merges (sm_sphere.hpp; smhip_sphere_merge): whole tensor: sphere_coefficients on the host; row-wise:
    // sphere_coef on the device.  Row data: row iterations | row flags ----
    int sphere_merge(const smhip_sphere_desc& d, void* out, float* delta_out, smhip_sphere_report* rep) {
        const int k = d.k;
        if (rep) *rep = smhip_sphere_report{};
        double A = 0.0;
        for (int i = 0; i < k; ++i) A = geo_dadd(A, d.alpha[i]);
        if (d.n == 0) return SMHIP_OK;

        GeoRun r;
        int rc;
        if ((rc = geo_begin("sphere_merge", d, out, delta_out, d.weight_space != 0, [](size_t R) { return 2 * round_up(R * sizeof(int), 256); }, r))) return rc;
        GeoCombineParams& m = r.m;
        GeoHead host;
        if (d.rowwise) {
            const size_t R = r.nseg;
            SphereCoefParams c;
            c.k = k; c.max_iter = d.max_iter; c.rows = R; c.tol = d.tol; c.A = A; c.G = r.part;
            for (int i = 0; i < TIES_MAX_MODELS; ++i) c.alpha[i] = d.alpha[i < k ? i : 0];
            c.coef = r.coef;
            c.iters = (int*)r.rows; c.flags = (int*)(r.rows + round_up(R * sizeof(int), 256));
            const int nt = sphere_coef_threads(k);
            if (k <= SPH_REG_SMALL) be.template launch<KSphereCoef>((int)((R + nt - 1) / nt), nt, sphere_coef_lds_floats(k) * 4, c, stream);
            else be.template launch<KSphereCoefLds>((int)((R + nt - 1) / nt), nt, sphere_coef_lds_floats(k) * 4, c, stream);
            m.rowcoef = c.coef;
            be.template launch<KGeoCombine>(r.cgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
            std::vector<float> coef(R * k);
            std::vector<int> iters(R), flags(R);
            be.d2h(coef.data(), c.coef, R * k * sizeof(float), stream);     // (the call's one synchronisation; the rest follows on the drained stream)
            be.d2h(iters.data(), c.iters, R * sizeof(int), stream);
            be.d2h(flags.data(), c.flags, R * sizeof(int), stream);
            if ((rc = geo_head("sphere_merge", k, r, host)) || !be.ok()) return rc;
            if (d.row_coef) std::copy(coef.begin(), coef.end(), d.row_coef);
            if (d.row_iters) std::copy(iters.begin(), iters.end(), d.row_iters);
            if (d.row_flags) std::copy(flags.begin(), flags.end(), d.row_flags);
            if (rep) {
                double sum = 0.0, lo = 0.0, hi = 0.0;
                for (size_t q = 0; q < R; ++q) {
                    double sr = 0.0;
                    for (int i = 0; i < k; ++i) sr = geo_dadd(sr, (double)coef[q * k + i]);
                    sum = geo_dadd(sum, sr);
                    lo = q ? std::min(lo, sr) : sr; hi = q ? std::max(hi, sr) : sr;
                    rep->iters_max = std::max(rep->iters_max, iters[q]);
                    rep->rows_unconverged += (flags[q] & SPH_CONVERGED) ? 0 : 1;
                    rep->rows_linear += (flags[q] & SPH_LINEAR) ? 1 : 0;
                }
                rep->csum_min = lo; rep->csum_max = hi; rep->csum_mean = geo_ddiv(sum, (double)R);
            }
            return SMHIP_OK;
        }

        if ((rc = geo_head("sphere_merge", k, r, host)) || !be.ok()) return rc;
        SphereRegs<TIES_MAX_MODELS> s;
        SphereOut o;
        sphere_coefficients<TIES_MAX_MODELS, false>(s, host.G, d.alpha, A, k, d.max_iter, d.tol, m.c, o);
        if (rep) {
            for (int i = 0; i < k; ++i) {
                for (int j = i; j < k; ++j) {
                    rep->G[i][j] = rep->G[j][i] = host.G[geo_pair_index(i, j, k)];
                    rep->H[i][j] = rep->H[j][i] = s.H(i, j);
                }
                rep->w[i] = s.w(i); rep->a[i] = s.a(i); rep->c[i] = m.c[i];
            }
            rep->N = o.N; rep->iterations = o.iterations; rep->tau = o.tau;
            rep->converged = (o.flags & SPH_CONVERGED) ? 1 : 0; rep->linear = (o.flags & SPH_LINEAR) ? 1 : 0;
        }
        be.template launch<KGeoCombine>(r.cgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
        return SMHIP_OK;
    }
    // the probe of an operator's defined functions: on the host, or one thread per argument on the device
    template <class KFn, class FnParams, class HostFn>
    int fn_array(HostFn host_fn, int op, const double* x, double* y, size_t n, bool on_device) {
        FnParams p;
        p.op = op; p.n = n; p.x = x; p.y = y;
        if (!on_device)
            for (size_t i = 0; i < n; ++i) y[i] = host_fn(op, x[i]);
        else if (n) be.template launch<KFn>((int)((n + 255) / 256), 256, LDS_SCRATCH_FLOATS * 4, p, stream);
        return SMHIP_OK;
    }
    int sphere_fn_array(int op, const double* x, double* y, size_t n, bool on_device) {      // sm_acos / sm_sin / sm_cos
        return fn_array<KSphereFn, SphereFnParams>([](int o, double v) { return sphere_fn(o, v); }, op, x, y, n, on_device);
    }

    // ---- SCE merge (sm_sce.hpp; smhip_sce_merge): the three levels of the ONE selection stream (skipped when
    // select_topk == 1 or k == 1), the energy pass and its fold, ONE readback (flags, the selection's results, the
    // energies), the weights on the host, the merge pass.  Workspace: select_workspace of one stream with SceHead as its
    // tail, then the segments' sums [nseg][k] ----
    struct SceHead { uint32_t flags[2]; SceState sel; double E[TIES_MAX_MODELS]; };
    int sce_merge(const smhip_sce_desc& d, void* out, float* delta_out, smhip_sce_report* rep) {
        const int k = d.k;
        const bool select = !(d.select_topk == 1.0 || k == 1);
        smhip_sce_report r{};
        auto weights = [&](const double* E, float* w) {           // step 3 on the host: one IEEE fp64 operation each
            double P[TIES_MAX_MODELS], Z = 0.0;
            for (int i = 0; i < k; ++i) { P[i] = geo_dmul(d.alpha[i], E[i]); Z = geo_dadd(Z, P[i]); }
            for (int i = 0; i < k; ++i) w[i] = (Z > 0.0 && geo_finite(Z)) ? (float)geo_ddiv(P[i], Z) : (float)geo_ddiv(1.0, (double)k);
        };
        if (d.n == 0) {                                  // nothing selected (k_keep == 0: the threshold is +inf), no energy
            r.threshold = select ? INFINITY : 0.f;
            weights(r.energy, r.weight);
            if (rep) *rep = r;
            return SMHIP_OK;
        }
        if (rep) *rep = r;
        SceMergeParams m;
        delta_inputs(d, out, delta_out, false, m);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.w[i] = 0.f;
        m.lambda = (float)d.lambda;
        const bool small = k <= SCE_REG_SMALL;
        const size_t nseg = (d.n + GEO_SEG_ELEMS - 1) / GEO_SEG_ELEMS;
        SceHead* head;
        size_t off_part;
        int rc;
        if ((rc = select_workspace(1, head, nseg * k * sizeof(double), &off_part))) return rc;
        m.select = select ? 1 : 0; m.state = &head->sel;

        if (select) {
            SceHistParams h;
            h.in = m.in; h.state = &head->sel; h.flags = head->flags;
            const int hgrid = hist_grid(h);
            SceSelectParams s;
            s.n = d.n; s.select_topk = d.select_topk; s.state = &head->sel;
            select_levels<KSceSelect>(1, 1, s, s, TIES_SELECT_LDS, [&](int level, unsigned long long* hist) {
                h.level = level; h.hist = hist;
                const size_t hlds = (LDS_SCRATCH_FLOATS + (size_t)radix_bins(level) + 1) * 4;     // (+ 1: the count of q == 0)
                if (small) be.template launch<KSceHist>(hgrid, 256, hlds, h, stream);
                else be.template launch<KSceHistAny>(hgrid, 256, hlds, h, stream);
            });
        }
        SceEnergyParams e;
        e.in = m.in; e.select = m.select; e.state = m.state; e.nseg = nseg; e.seg_vec = m.in.aligned;
        e.part = (double*)ws_at(off_part); e.flags = head->flags;
        if (small) be.template launch<KSceEnergy>((int)nseg, GEO_THREADS, sce_energy_lds_floats<SCE_REG_SMALL>() * 4, e, stream);
        else be.template launch<KSceEnergyAny>((int)nseg, GEO_THREADS, sce_energy_lds_floats<TIES_MAX_MODELS>() * 4, e, stream);
        fold_pass<KSceFold>(k, nseg, e.part, head->E);

        SceHead host;
        if ((rc = delta_readback("sce_merge", k, head, host))) return rc;     // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;                        // (reported by the caller as SMHIP_ERR_HIP; the report stays zero)
        if (select) {
            r.nz = d.n - host.sel.zeros; r.k_keep = host.sel.k_keep; r.selected = host.sel.selected; r.threshold = host.sel.threshold;
        } else {                                             // every element is selected: every q >= +0 reaches a threshold of 0
            r.nz = r.k_keep = r.selected = d.n; r.threshold = 0.f;
        }
        for (int i = 0; i < k; ++i) r.energy[i] = host.E[i];
        weights(r.energy, r.weight);
        for (int i = 0; i < k; ++i) m.w[i] = r.weight[i];
        if (rep) *rep = r;
        const int mgrid = stream_grid((d.n + 7) / 8, 256, m.chunks);
        if (small) be.template launch<KSceMerge>(mgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
        else be.template launch<KSceMergeAny>(mgrid, 256, LDS_SCRATCH_FLOATS * 4, m, stream);
        return SMHIP_OK;
    }

    // ---- DELLA merge (sm_della.hpp; smhip_della_merge).  epsilon == 0 or density == 1: the uniform threshold, dare_pass
    // itself.  Otherwise slabs of whole rows: rank all k finetunes of a slab into the workspace, merge the slab; the mask
    // index stays the flat index in the tensor.  Workspace: DareReadback | the table T(rank) [c] | uint16 [k][stride] ----
    static constexpr size_t DELLA_SLAB_ELEMS = (size_t)1 << 26;
    int della_merge(const smhip_della_desc& d, void* out, float* delta_out, uint16_t* threshold_out, smhip_della_report* rep) {
        const int k = d.k;
        const bool uniform = d.epsilon == 0.0 || d.density == 1.0;
        const double p_lo = d.density - d.epsilon, w = 2.0 * d.epsilon;
        const size_t c = d.n ? d.n / d.rows : 1;
        const uint32_t T_lo = uniform ? dare_threshold(d.density) : della_threshold(p_lo, w, 0u, (uint32_t)c);
        const uint32_t T_hi = uniform ? T_lo : della_threshold(p_lo, w, (uint32_t)(c - 1), (uint32_t)c);
        if (rep) {
            rep->T_lo = T_lo; rep->T_hi = T_hi;
            for (int i = 0; i < SMHIP_MAX_MODELS; ++i) rep->kept[i] = 0;
        }
        if (d.n == 0) return SMHIP_OK;
        uint64_t* kept = rep ? rep->kept : nullptr;
        int rc;
        if (uniform) {
            if (threshold_out && d.density < 1.0) {
                DellaTableParams t;
                t.out = threshold_out; t.count = (size_t)k * d.n; t.c = 1; t.p_lo = 0.0; t.w = 0.0; t.fill = T_lo;
                if ((t.count + 255) / 256 > (size_t)0x7fffffff) return fail(SMHIP_ERR_ARG, "della_merge: tensor too large for threshold_out");
                be.template launch<KDellaTable>((int)((t.count + 255) / 256), 256, LDS_SCRATCH_FLOATS * 4, t, stream);
            }
            return dare_pass("della_merge", d, T_lo, out, delta_out, kept);
        }
        const size_t R = d.rows;
        size_t slab_rows = della_slab_rows ? della_slab_rows : std::max<size_t>(1, DELLA_SLAB_ELEMS / c);
        slab_rows = std::min(slab_rows, std::min<size_t>(R, (size_t)0x7fffffff / TIES_MAX_MODELS));
        const size_t stride = round_up(7 + slab_rows * c, 8);
        const size_t off_table = round_up(sizeof(DareReadback), 256), off_ws = off_table + round_up(c * sizeof(uint16_t), 256);
        DareReadback* rb;
        if ((rc = plain_workspace(rb, off_ws + (size_t)k * stride * sizeof(uint16_t)))) return rc;

        DellaTableParams t;
        t.out = (uint16_t*)ws_at(off_table); t.count = c; t.c = (uint32_t)c; t.p_lo = p_lo; t.w = w; t.fill = 0;
        be.template launch<KDellaTable>((int)((c + 255) / 256), 256, LDS_SCRATCH_FLOATS * 4, t, stream);

        DellaMergeParams m;
        delta_merge_params(d, out, delta_out, m);
        dare_fields(d, rb, m);
        m.rescale = d.rescale ? 1 : 0;
        DellaRankParams r;
        r.in = m.in; r.c = (int)c; r.table = t.out; r.threshold_out = threshold_out; r.flags = rb->flags;
        r.P = 8;
        while ((size_t)r.P < c) r.P <<= 1;
        const int rank_threads = std::min(1024, std::max(64, r.P / 8));
        for (size_t r0 = 0; r0 < R; r0 += slab_rows) {
            const size_t rows = std::min(slab_rows, R - r0);
            DellaSlab s;
            s.e0 = r0 * c; s.len = rows * c; s.stride = stride; s.ws = (uint16_t*)ws_at(off_ws);
            r.slab = s; r.rows = (int)rows;
            be.template launch<KDellaRank>((int)(rows * k), rank_threads, (LDS_SCRATCH_FLOATS + (size_t)r.P) * 4, r, stream);
            m.slab = s;
            const size_t noct = ((s.e0 + s.len + 7) >> 3) - (s.e0 >> 3);
            m.chunks = pick_chunks(noct, 256, 2, 8);
            be.template launch<KDellaMerge>(stream_grid(noct, 256, m.chunks), 256, (LDS_SCRATCH_FLOATS + dare_lds_words(k, 256)) * 4, m, stream);
        }
        return dare_readback("della_merge", k, rb, kept);
    }

    // ---- Consensus merge (sm_consensus.hpp; smhip_consensus_merge).  ties == 0: no select, one kernel, the workspace is
    // ConsensusWork alone.  ties == 1: the thresholds of TIES (select_workspace with ConsensusWork as its tail), then the
    // one kernel ----
    struct ConsensusReadback {
        float threshold[TIES_MAX_MODELS];
        unsigned long long kept[TIES_MAX_MODELS], masked[TIES_MAX_MODELS], counts[CONSENSUS_COUNTS];
        uint32_t flags[2];
    };
    struct ConsensusWork { RadixState state[TIES_MAX_MODELS]; ConsensusReadback rb; };
    int consensus_merge(const smhip_consensus_desc& d, void* out, float* delta_out, smhip_consensus_report* rep) {
        const int k = d.k;
        const bool ties = d.ties != 0;
        const unsigned long long k_keep = ties ? delta_k_keep(d.density, d.n) : 0ull;
        if (rep) {
            *rep = smhip_consensus_report{};
            rep->k_keep = k_keep;
        }
        if (d.n == 0) {                                  // (ties, k_keep == 0: the threshold is +inf by definition)
            if (rep && ties) for (int i = 0; i < k; ++i) rep->threshold[i] = INFINITY;
            return SMHIP_OK;
        }
        ConsensusWork* w;
        int rc;
        if ((rc = ties ? select_workspace(TIES_MAX_MODELS, w) : plain_workspace(w))) return rc;

        ConsensusMergeParams m;
        delta_merge_params(d, out, delta_out, m);
        m.ties = ties ? 1 : 0; m.threshold = w->rb.threshold;
        m.mask_lambda = (float)d.mask_lambda; m.need = (uint32_t)std::min(d.consensus_k, k);
        m.masked = w->rb.masked; m.counts = w->rb.counts; m.flags = w->rb.flags;

        if (ties) ties_thresholds(m.in, k_keep, w);
        const int grid = stream_grid((d.n + 7) / 8, 256, m.chunks);
        const size_t lds = (LDS_SCRATCH_FLOATS + consensus_lds_words(k, 256)) * 4;
        if (k <= CONSENSUS_REG_SMALL) be.template launch<KConsensusMerge>(grid, 256, lds, m, stream);
        else be.template launch<KConsensusMergeAny>(grid, 256, lds, m, stream);

        ConsensusReadback host;
        if ((rc = delta_readback("consensus_merge", k, &w->rb, host))) return rc;     // the call's one synchronisation
        if (rep) {
            for (int i = 0; i < k; ++i) {
                if (ties) { rep->threshold[i] = host.threshold[i]; rep->kept[i] = host.kept[i]; }
                rep->masked[i] = host.masked[i];
            }
            for (int c = 0; c <= TIES_MAX_MODELS; ++c) rep->agree[c] = host.counts[c];
            rep->selected = host.counts[TIES_MAX_MODELS + 1];
        }
        return SMHIP_OK;
    }

    // ---- Pairwise fusion (sm_fusion.hpp; smhip_fusion_merge).  NEARSWAP: one kernel, the workspace is FusionWork alone.
    // ARCEE: the row KL, the three levels of the three-rank select over the score stream, the gate pass, ONE readback.
    // Workspace: the histograms [3][STATS_HIST_STRIDE] | FusionWork | kappa [R] when the caller gives no kl_out ----
    struct FusionReadback {
        float tau[STATS_MAX_RANKS * TIES_MAX_MODELS];                  // stats_select's layout: Q_q at [q * TIES_MAX_MODELS]
        unsigned long long kept[STATS_MAX_RANKS * TIES_MAX_MODELS];    // (stats_select's kept counts: not reported)
        unsigned long long count;                                      // selected / clipped
        float threshold;
        uint32_t kl_minmax[2];
        uint32_t flags[2];
    };
    struct FusionWork { RadixState state[STATS_MAX_RANKS]; FusionReadback rb; };
    int fusion_nonfinite(uint32_t flags) {
        std::string which;
        if (flags & FUS_BAD_FT) which = "the finetune";
        if (flags & FUS_BAD_BASE) which += std::string(which.empty() ? "" : " and ") + "the base";
        if (which.empty()) which = "finetune - base";
        return fail(SMHIP_ERR_NONFINITE, "fusion_merge: NaN or Inf in " + which);
    }
    int fusion_merge(const smhip_fusion_desc& d, void* out, float* delta_out, smhip_fusion_report* rep) {
        const bool arcee = d.mode == SMHIP_FUSION_ARCEE;
        if (rep) *rep = smhip_fusion_report{};
        if (d.n == 0) return SMHIP_OK;
        const size_t n = d.n, R = d.rows, C = n / R;
        if (arcee && R > (size_t)0x7fffffff) return fail(SMHIP_ERR_ARG, "fusion_merge: too many rows");
        FusionMergeParams m;
        delta_inputs(d, out, delta_out, false, m);
        m.C = C; m.kl = nullptr; m.quart = nullptr; m.threshold = nullptr;
        m.iqr_mult = (float)d.iqr_mult; m.t = (float)d.t;
        const int grid = stream_grid((n + 7) / 8, 256, m.chunks);
        const size_t merge_lds = (LDS_SCRATCH_FLOATS + 4) * 4;
        FusionWork* w;
        int rc;
        if (!arcee) {
            if ((rc = plain_workspace(w))) return rc;
            m.count = &w->rb.count; m.flags = w->rb.flags;
            be.template launch<KFusionMergeNear>(grid, 256, merge_lds, m, stream);
        } else {
            size_t off_kl = 0;
            if ((rc = select_workspace(2, w, d.kl_out ? 0 : R * sizeof(float), &off_kl))) return rc;
            float* kl = d.kl_out ? d.kl_out : (float*)ws_at(off_kl);
            FusionRowKlParams k;
            k.ft = m.in.ft[0]; k.base = m.in.base[0]; k.dtype = m.in.dtype; k.C = C;
            k.seg_vec = (aligned16(k.ft) && aligned16(k.base) && C % 8 == 0) ? 1 : 0;
            k.kl = kl; k.flags = w->rb.flags;
            be.template launch<KFusionRowKl>((int)R, GEO_THREADS, fusion_rowkl_lds_floats() * 4, k, stream);

            FusionHistParams h;
            h.in = m.in; h.C = C; h.kl = kl; h.state = w->state;
            const int hgrid = hist_grid(h);
            FusionSelectParams s;
            s.sel.m = FUS_RANKS; s.sel.state = w->state; s.sel.tau = w->rb.tau; s.sel.kept = w->rb.kept;
            // rho_q = floor(q (n - 1)), q = 1/4, 1/2, 3/4, in integers; the rho-th smallest is the (n - rho)-th largest
            const unsigned long long n1 = (unsigned long long)n - 1;
            const unsigned long long rho[FUS_RANKS] = {n1 / 4, n1 / 2, 3 * n1 / 4};      // (n <= 2^41: delta_tensor_check)
            for (int q = 0; q < STATS_MAX_RANKS; ++q) s.sel.rank[q] = (unsigned long long)n - rho[q < FUS_RANKS ? q : 0];
            s.rows = R; s.kl = kl; s.kl_minmax = w->rb.kl_minmax;
            select_levels<KFusionSelect>(2, 1, s, s.sel, FUSION_SELECT_LDS, [&](int level, unsigned long long* hist) {
                h.level = level; h.hist = hist;
                be.template launch<KFusionHist>(hgrid, 256, (LDS_SCRATCH_FLOATS + (size_t)fusion_hist_words(level)) * 4, h, stream);
            });
            m.kl = kl; m.quart = w->rb.tau; m.threshold = &w->rb.threshold;
            m.count = &w->rb.count; m.flags = w->rb.flags;
            be.template launch<KFusionMergeArcee>(grid, 256, merge_lds, m, stream);
        }
        FusionReadback host;
        be.d2h(&host, &w->rb, sizeof host, stream);      // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;
        if (host.flags[0]) return fusion_nonfinite(host.flags[0]);
        if (rep) {
            if (arcee) {
                rep->q1 = host.tau[0]; rep->q2 = host.tau[TIES_MAX_MODELS]; rep->q3 = host.tau[2 * TIES_MAX_MODELS];
                rep->threshold = host.threshold; rep->selected = host.count;
                rep->kl_min = u2f(host.kl_minmax[0]); rep->kl_max = u2f(host.kl_minmax[1]);
            } else {
                rep->clipped = host.count;
            }
        }
        return SMHIP_OK;
    }
    int fusion_fn_array(int op, const double* x, double* y, size_t n, bool on_device) {      // sm_exp / sm_log
        return fn_array<KFusionFn, FusionFnParams>([](int o, double v) { return fusion_fn(o, v); }, op, x, y, n, on_device);
    }

    // ---- PCB merge (sm_pcb.hpp; smhip_pcb_merge): the clip's two order statistics per finetune (stats_hist / stats_select
    // with m = 2, unchanged), the histograms zeroed again, the three levels of the two-rank select over the score stream
    // (pcb_hist, stats_select), the fused pass, ONE readback.  Workspace: select_workspace of stats' 32 streams with
    // PcbWork as its tail ----
    struct PcbReadback {
        float q[STATS_MAX_RANKS * TIES_MAX_MODELS];                    // stats_select's layout: rank r of |d_i| at [r * TIES_MAX_MODELS + i]
        unsigned long long q_kept[STATS_MAX_RANKS * TIES_MAX_MODELS];  // (its kept counts: not reported)
        float tm[STATS_MAX_RANKS * TIES_MAX_MODELS];                   // M_i at [PCB_MAX], t_i at [PCB_CUT]
        unsigned long long tm_kept[STATS_MAX_RANKS * TIES_MAX_MODELS]; // at [PCB_CUT]: selected[i]
        float bounds[2 * TIES_MAX_MODELS];                             // lo_i, then hi_i
        unsigned long long positive[TIES_MAX_MODELS], counts[PCB_COUNTS];
        uint32_t flags[2];
    };
    struct PcbWork { RadixState clip[STATS_MAX_RANKS * TIES_MAX_MODELS], score[STATS_MAX_RANKS * TIES_MAX_MODELS]; PcbReadback rb; };
    int pcb_merge(const smhip_pcb_desc& d, void* out, float* delta_out, smhip_pcb_report* rep) {
        const int k = d.k;
        const unsigned long long n = d.n;
        const unsigned long long r = (unsigned long long)std::floor(d.clip * (double)n);
        const unsigned long long q = d.ratio == 1.0 ? n : std::max(1ull, (unsigned long long)std::floor(d.ratio * (double)n));
        if (rep) {
            *rep = smhip_pcb_report{};
            rep->clip_rank = r; rep->q = n ? q : 0;
        }
        if (n == 0) return SMHIP_OK;
        const int streams = 2 * TIES_MAX_MODELS;
        PcbWork* w;
        int rc;
        if ((rc = select_workspace(streams, w))) return rc;

        PcbMergeParams m;
        delta_inputs(d, out, delta_out, false, m);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.alpha[i] = (float)d.alpha[i < k ? i : 0];
        m.lambda = (float)d.lambda;
        m.q = w->rb.q; m.tm = w->rb.tm; m.bounds = w->rb.bounds; m.positive = w->rb.positive; m.counts = w->rb.counts;

        // step 2: the (r + 1)-th largest and the (n - r)-th largest |d_i|
        StatsHistParams h;
        h.in = m.in; h.m = PCB_RANKS; h.state = w->clip; h.flags = w->rb.flags;
        StatsSelectParams s;
        s.m = PCB_RANKS; s.state = w->clip; s.tau = w->rb.q; s.kept = w->rb.q_kept;
        for (int j = 0; j < STATS_MAX_RANKS; ++j) s.rank[j] = j == PCB_LO ? n - r : r + 1;
        select_levels_per_finetune<KStatsHist, KStatsSelect>(streams, h, s, STATS_SELECT_LDS,
                                                             [](int level) { return stats_hist_words(level, PCB_RANKS); }, false);
        be.memset(ws_.p, 0, 3 * select_hist_level(streams), stream);

        // step 6: the largest and the q-th largest score
        PcbHistParams ph;
        ph.in = m.in; ph.q = w->rb.q; ph.state = w->score;
        for (int i = 0; i < TIES_MAX_MODELS; ++i) ph.alpha[i] = m.alpha[i];
        const int hgrid = hist_grid(ph);
        const bool small = k <= PCB_REG_SMALL;
        StatsSelectParams ss;
        ss.m = PCB_RANKS; ss.state = w->score; ss.tau = w->rb.tm; ss.kept = w->rb.tm_kept;
        for (int j = 0; j < STATS_MAX_RANKS; ++j) ss.rank[j] = j == PCB_CUT ? q : 1ull;
        select_levels<KStatsSelect>(streams, k, ss, ss, STATS_SELECT_LDS, [&](int level, unsigned long long* hist) {
            ph.level = level; ph.hist = hist;
            for (int first = 0; first < k; first += TIES_GROUP) {
                ph.first = first; ph.count = std::min(TIES_GROUP, k - first);
                const size_t lds = (LDS_SCRATCH_FLOATS + pcb_hist_lds_words(level, ph.count)) * 4;
                if (small) be.template launch<KPcbHist>(hgrid, 256, lds, ph, stream);
                else be.template launch<KPcbHistAny>(hgrid, 256, lds, ph, stream);
            }
        });

        const int grid = stream_grid((d.n + 7) / 8, 256, m.chunks);
        const size_t lds = (LDS_SCRATCH_FLOATS + pcb_merge_lds_words(k, 256)) * 4;
        if (small) be.template launch<KPcbMerge>(grid, 256, lds, m, stream);
        else be.template launch<KPcbMergeAny>(grid, 256, lds, m, stream);

        PcbReadback host;
        if ((rc = delta_readback("pcb_merge", k, &w->rb, host))) return rc;      // the call's one synchronisation
        if (rep) {
            for (int i = 0; i < k; ++i) {
                rep->lo[i] = host.bounds[i]; rep->hi[i] = host.bounds[TIES_MAX_MODELS + i];
                rep->M[i] = host.tm[PCB_MAX * TIES_MAX_MODELS + i]; rep->t[i] = host.tm[PCB_CUT * TIES_MAX_MODELS + i];
                rep->positive[i] = host.positive[i]; rep->selected[i] = host.tm_kept[PCB_CUT * TIES_MAX_MODELS + i];
            }
            rep->covered = host.counts[PCB_COVERED]; rep->contested = host.counts[PCB_CONTESTED];
        }
        return SMHIP_OK;
    }
    int pcb_fn_array(int op, const double* x, double* y, size_t n, bool on_device) {         // sm_tanh
        return fn_array<KPcbFn, PcbFnParams>([](int o, double v) { return pcb_fn(o, v); }, op, x, y, n, on_device);
    }

    // ---- WIDEN merge (sm_widen.hpp; smhip_widen_merge): the column sums and their fold (vector mode: the fold alone, from
    // the inputs), the ranks, the weights, the combine pass, ONE readback.  Workspace: WidenHead (zeroed) | the partials
    // [nseg][k][3][C] | the statistics [k][2][C] | the ranks [k][2][C] | the weights [k][C]; an optional output of the
    // call takes the place of its workspace array ----
    struct WidenHead {
        uint32_t flags[2];
        unsigned long long ranksum[TIES_MAX_MODELS * WIDEN_STATS], calibrated[TIES_MAX_MODELS * WIDEN_STATS];
        double mu[TIES_MAX_MODELS * WIDEN_STATS];
    };
    int widen_merge(const smhip_widen_desc& d, void* out, float* delta_out, double* stat_out, uint32_t* rank_out,
                    float* weight_out, smhip_widen_report* rep) {
        const int k = d.k;
        if (rep) *rep = smhip_widen_report{};
        if (d.n == 0) return SMHIP_OK;
        const size_t R = d.rows, C = d.n / d.rows;
        const bool vector_mode = R == 1;
        const int ns = vector_mode ? 1 : WIDEN_STATS;
        if (rep) { rep->rows = R; rep->cols = C; rep->vector_mode = vector_mode ? 1 : 0; }
        const size_t nseg = (R + WIDEN_SEG_ROWS - 1) / WIDEN_SEG_ROWS, ncb = (C + WIDEN_COLS - 1) / WIDEN_COLS;
        if (nseg * ncb * (size_t)k > (size_t)0x7fffffff) return fail(SMHIP_ERR_ARG, "widen_merge: tensor too large");

        const size_t off_part = round_up(sizeof(WidenHead), 256);
        const size_t part_bytes = vector_mode ? 0 : round_up(nseg * k * WIDEN_SUMS * C * sizeof(double), 256);
        const size_t off_stat = off_part + part_bytes, stat_bytes = round_up((size_t)k * WIDEN_STATS * C * sizeof(double), 256);
        const size_t off_rank = off_stat + stat_bytes, rank_bytes = round_up((size_t)k * WIDEN_STATS * C * sizeof(uint32_t), 256);
        const size_t off_weight = off_rank + rank_bytes, weight_bytes = round_up((size_t)k * C * sizeof(float), 256);
        WidenHead* head;
        int rc;
        if ((rc = plain_workspace(head, off_weight + weight_bytes))) return rc;
        double* stat = stat_out ? stat_out : (double*)ws_at(off_stat);
        uint32_t* rank = rank_out ? rank_out : (uint32_t*)ws_at(off_rank);
        float* weight = weight_out ? weight_out : (float*)ws_at(off_weight);

        WidenCombineParams m;
        delta_inputs(d, out, delta_out, false, m);
        m.R = R; m.C = C; m.ncb = (int)ncb; m.vec = (m.in.aligned && C % 8 == 0) ? 1 : 0;
        m.weight = weight; m.lambda = (float)d.lambda;
        // about eight work-groups per CU, each thread at least one row
        const size_t row_blocks = std::max<size_t>(1, std::min<size_t>((R + WIDEN_SUB - 1) / WIDEN_SUB, (2048 + ncb - 1) / ncb));
        m.rows_per_wg = (int)round_up((R + row_blocks - 1) / row_blocks, WIDEN_SUB);
        const size_t cgrid = ncb * ((R + m.rows_per_wg - 1) / m.rows_per_wg);

        WidenColfoldParams f;
        f.in = m.in; f.C = C; f.nseg = (int)nseg; f.vector_mode = vector_mode ? 1 : 0;
        f.part = (const double*)ws_at(off_part); f.stat = stat; f.flags = head->flags;
        if (!vector_mode) {
            WidenColstatsParams c;
            c.in = m.in; c.R = R; c.C = C; c.nseg = (int)nseg; c.ncb = (int)ncb; c.vec = m.vec;
            c.part = (double*)ws_at(off_part);
            be.template launch<KWidenColstats>((int)(nseg * ncb * k), WIDEN_THREADS, widen_colstats_lds_floats() * 4, c, stream);
        }
        const int col_blocks = (int)((C + 255) / 256);
        be.template launch<KWidenColfold>(col_blocks * k, 256, LDS_SCRATCH_FLOATS * 4, f, stream);

        WidenRankParams r;
        r.C = C; r.ns = ns; r.stat = stat; r.rank = rank; r.ranksum = head->ranksum;
        be.memset(rank, 0, (size_t)k * WIDEN_STATS * C * sizeof(uint32_t), stream);
        be.template launch<KWidenRank>(col_blocks * k * WIDEN_STATS * widen_rank_tiles(C), 256, widen_rank_lds_floats() * 4, r, stream);

        WidenCoefParams w;
        w.k = k; w.C = C; w.ns = ns; w.ratio = d.ratio; w.calibration = d.calibration;
        for (int i = 0; i < TIES_MAX_MODELS; ++i) w.alpha[i] = d.alpha[i < k ? i : 0];
        w.rank = rank; w.ranksum = head->ranksum; w.weight = weight; w.mu = head->mu; w.calibrated = head->calibrated;
        be.template launch<KWidenCoef>(col_blocks, 256, widen_coef_lds_floats() * 4, w, stream);

        if (k <= WIDEN_REG_SMALL) be.template launch<KWidenCombine>((int)cgrid, WIDEN_THREADS, LDS_SCRATCH_FLOATS * 4, m, stream);
        else be.template launch<KWidenCombineAny>((int)cgrid, WIDEN_THREADS, LDS_SCRATCH_FLOATS * 4, m, stream);

        WidenHead host;
        be.d2h(&host, head, sizeof host, stream);                  // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;                             // (reported by the caller as SMHIP_ERR_HIP)
        if (host.flags[0]) return delta_nonfinite("widen_merge", vector_mode ? "finetune - base" : "the finetune or the base", k, host.flags[0]);
        if (rep)
            for (int i = 0; i < k; ++i)
                for (int s = 0; s < WIDEN_STATS; ++s) {
                    rep->mu[i][s] = host.mu[i * WIDEN_STATS + s];
                    rep->calibrated[i][s] = host.calibrated[i * WIDEN_STATS + s];
                }
        return SMHIP_OK;
    }

    // ---- CABS merge (sm_cabs.hpp; smhip_cabs_merge): no select launch, one kernel; the workspace is CabsReadback ----
    struct CabsReadback { unsigned long long kept[TIES_MAX_MODELS], counts[CABS_COUNTS]; uint32_t flags[2]; };
    int cabs_merge(const smhip_cabs_desc& d, void* out, float* delta_out, uint16_t* mask_out, smhip_cabs_report* rep) {
        const int k = d.k, M = d.group;
        if (rep) *rep = smhip_cabs_report{};
        if (d.n == 0) return SMHIP_OK;
        const size_t R = d.rows, C = d.n / R;
        const size_t Mu = (size_t)std::max(M, 8);
        CabsMergeParams m;
        delta_inputs(d, out, delta_out, false, m);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.alpha[i] = (float)d.alpha[i < k ? i : 0];
        m.lambda = (float)d.lambda;
        m.mask_out = mask_out;
        m.R = R; m.C = C; m.G = (C + Mu - 1) / Mu;
        m.M = M; m.N = d.n_keep; m.L = (int)(Mu / 8);
        m.log2L = 0;
        while ((1 << m.log2L) < m.L) ++m.log2L;
        m.conflict_aware = d.conflict_aware ? 1 : 0;
        m.row_vec = (m.in.aligned && C % 8 == 0 && aligned16(mask_out)) ? 1 : 0;
        // every row octet of every team, the idle ones of the tail groups included: at most n / 8 + R * M / 8
        if (R > ((size_t)1 << 56) / (m.G * (size_t)m.L)) return fail(SMHIP_ERR_ARG, "cabs_merge: tensor too large");
        m.units = R * m.G * (size_t)m.L;
        m.chunks = pick_chunks(m.units, CABS_THREADS, 2, 8);
        if ((m.units + CABS_THREADS - 1) / CABS_THREADS / (size_t)m.chunks > (size_t)0x7fffffff) return fail(SMHIP_ERR_ARG, "cabs_merge: tensor too large");
        CabsReadback* rb;
        int rc;
        if ((rc = plain_workspace(rb))) return rc;
        m.kept = rb->kept; m.counts = rb->counts; m.flags = rb->flags;

        const int grid = stream_grid(m.units, CABS_THREADS, m.chunks);
        const size_t lds = (LDS_SCRATCH_FLOATS + cabs_lds_words(k, m.L, CABS_THREADS)) * 4;
        if (k <= CABS_REG_SMALL) be.template launch<KCabsMerge>(grid, CABS_THREADS, lds, m, stream);
        else be.template launch<KCabsMergeAny>(grid, CABS_THREADS, lds, m, stream);

        CabsReadback host;
        if ((rc = delta_readback("cabs_merge", k, rb, host))) return rc;     // the call's one synchronisation
        if (rep) {
            rep->groups = (uint64_t)R * (uint64_t)((C + (size_t)M - 1) / (size_t)M);
            for (int i = 0; i < k; ++i) {
                rep->kept[i] = host.kept[i];
                rep->short_groups[i] = host.counts[i];
                rep->surplus[i] = host.counts[TIES_MAX_MODELS + i];
            }
            rep->covered = host.counts[2 * TIES_MAX_MODELS];
            rep->overlap = host.counts[2 * TIES_MAX_MODELS + 1];
        }
        return SMHIP_OK;
    }

    // ---- Task-vector statistics (sm_stats.hpp; smhip_delta_stats): the three selection levels for every density at once,
    // the Gram pass and its fold, the one fused pass and its fold, ONE readback.  Workspace: the histograms
    // [3][32][HIST1_BINS] (STATS_HIST_STRIDE words per finetune) | StatsWork | the Gram's partials | the energies' partials ----
    struct StatsReadback {
        float tau[STATS_MAX_RANKS * TIES_MAX_MODELS];
        unsigned long long kept[STATS_MAX_RANKS * TIES_MAX_MODELS];
        double energy[STATS_MAX_RANKS * TIES_MAX_MODELS];
        double G[TIES_MAX_MODELS * (TIES_MAX_MODELS + 1) / 2];
        unsigned long long counts[STATS_COUNTS];
        uint32_t flags[2];
    };
    struct StatsWork { RadixState state[STATS_MAX_RANKS * TIES_MAX_MODELS]; StatsReadback rb; };
    int delta_stats(const smhip_stats_desc& d, smhip_stats_report* rep) {
        const int k = d.k, m = d.m;
        *rep = smhip_stats_report{};
        for (int q = 0; q < m; ++q) {
            rep->k_keep[q] = delta_k_keep(d.density[q], d.n);
            if (d.n == 0) for (int i = 0; i < k; ++i) rep->tau[q][i] = INFINITY;     // k_keep == 0: +inf by definition
        }
        if (d.n == 0) return SMHIP_OK;

        TiesInputs in;
        ties_inputs(in, k, d.in_dtype, d.n, d.finetune, d.base, true);
        const size_t nseg = (d.n + GEO_SEG_ELEMS - 1) / GEO_SEG_ELEMS;
        const size_t gram_bytes = round_up(nseg * geo_pairs(k) * sizeof(double), 256);
        StatsWork* w;
        size_t off_part;
        int rc;
        if ((rc = gram_grid("delta_stats", k, nseg))) return rc;
        if ((rc = select_workspace(2 * TIES_MAX_MODELS, w, gram_bytes + nseg * m * k * sizeof(double), &off_part))) return rc;

        StatsHistParams h;
        h.in = in; h.m = m; h.state = w->state; h.flags = w->rb.flags;
        StatsSelectParams s;
        s.m = m; s.state = w->state; s.tau = w->rb.tau; s.kept = w->rb.kept;
        for (int q = 0; q < STATS_MAX_RANKS; ++q) s.rank[q] = rep->k_keep[q < m ? q : 0];
        select_levels_per_finetune<KStatsHist, KStatsSelect>(2 * TIES_MAX_MODELS, h, s, STATS_SELECT_LDS,
                                                             [m](int level) { return stats_hist_words(level, m); }, false);
        gram_pass(in, false, GEO_SEG_ELEMS, nseg, (double*)ws_at(off_part), w->rb.flags, w->rb.G);

        StatsPassParams sp;
        sp.in = in; sp.m = m; sp.tau = w->rb.tau; sp.nseg = nseg; sp.seg_vec = in.aligned;
        for (int i = 0; i < TIES_MAX_MODELS; ++i) sp.alpha[i] = (float)d.alpha[i < k ? i : 0];
        sp.part = (double*)ws_at(off_part + gram_bytes); sp.counts = w->rb.counts;
        if (k <= STATS_REG_SMALL) be.template launch<KStatsPass>((int)nseg, GEO_THREADS, stats_pass_lds_floats(m, k) * 4, sp, stream);
        else be.template launch<KStatsPassAny>((int)nseg, GEO_THREADS, stats_pass_lds_floats(m, k) * 4, sp, stream);
        fold_pass<KStatsFold>(m * k, nseg, sp.part, w->rb.energy, k, TIES_MAX_MODELS);

        StatsReadback host;
        if ((rc = delta_readback("delta_stats", k, &w->rb, host))) return rc;       // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;
        const unsigned long long* c = host.counts;
        for (int i = 0; i < k; ++i) {
            rep->nonzero[i] = c[STATS_NONZERO + i];
            for (int j = i; j < k; ++j) rep->G[i][j] = rep->G[j][i] = host.G[geo_pair_index(i, j, k)];
        }
        for (int q = 0; q < m; ++q) {
            for (int i = 0; i < k; ++i) {
                const int qi = q * TIES_MAX_MODELS + i;
                rep->tau[q][i] = host.tau[qi]; rep->kept[q][i] = host.kept[qi]; rep->energy[q][i] = host.energy[qi];
                rep->opposed[q][i] = c[STATS_OPPOSED + qi]; rep->alone[q][i] = c[STATS_ALONE + qi];
            }
            for (int cc = 0; cc <= k; ++cc) rep->cover[q][cc] = c[STATS_COVER + q * (TIES_MAX_MODELS + 1) + cc];
            rep->conflict[q] = c[STATS_CONFLICT + q];
        }
        return SMHIP_OK;
    }

    // ---- Low-rank extraction (sm_extract.hpp; smhip_lora_extract).  The caller's workspace: two panels
    // [max(rows, cols) x L] | the delta product's partials | the Gram's partials | G | T | the energy's partials | its sum
    // and the flags ----
    struct XlLayout {
        int L;
        size_t pan, part, gpart, G, T, epart, tail, total;      // byte offsets; pan: the size of one panel
        size_t eseg;
    };
    static XlLayout xl_layout_L(int rows, int cols, int L_, int tcols) {
        XlLayout y;
        y.L = L_;
        const size_t mx = (size_t)std::max(rows, cols), L = (size_t)y.L;
        auto nseg = [](int K) { return (size_t)(K + XL_SEG - 1) / XL_SEG; };
        y.pan = round_up(mx * L * 4, 256);
        const size_t part = std::max(nseg(cols) * (size_t)rows, nseg(rows) * (size_t)cols) * L * 4;
        const size_t gpart = (mx + XL_GSEG - 1) / XL_GSEG * L * L * 8;
        y.eseg = ((size_t)rows * cols + GEO_SEG_ELEMS - 1) / GEO_SEG_ELEMS;
        y.part = 2 * y.pan;
        y.gpart = y.part + round_up(part, 256);
        y.G = y.gpart + round_up(gpart, 256);
        y.T = y.G + round_up(L * L * 8, 256);
        y.epart = y.T + round_up(2 * L * (size_t)std::max(y.L, tcols) * 4, 256);     // T [L x L], or Tb and Ta [L x r]
        y.tail = y.epart + round_up(y.eseg * 8, 256);
        y.total = y.tail + 256;
        return y;
    }
    static XlLayout xl_layout(int rows, int cols, int rank) { return xl_layout_L(rows, cols, xl_panel_width(rows, cols, rank), rank); }
    void xl_delta_mm(const void* ft, const void* base, int dtype, int rows, int cols, int trans, int L, const float* x,
                     float* out, void* ws, const XlLayout& y) {
        const int M = trans ? cols : rows, K = trans ? rows : cols, MT = trans ? XL_MT1 : XL_MT0;
        XlMmParams m;
        m.ft = ft; m.base = base; m.dtype = dtype; m.rows = rows; m.cols = cols; m.trans = trans; m.L = L; m.x = x;
        m.part = (float*)((char*)ws + y.part);
        m.nseg = (K + XL_SEG - 1) / XL_SEG; m.nchunk = (L / 16 + XL_CT - 1) / XL_CT;
        m.vec = (aligned16(ft) && aligned16(base) && cols % 8 == 0) ? 1 : 0;
        const size_t grid = (size_t)((M + MT - 1) / MT) * m.nseg * m.nchunk;
        be.template launch<KXlDeltaMm>((int)grid, 64, 0, m, stream);
        XlFoldParams f;
        f.part = m.part; f.out = out; f.n = (size_t)M * L; f.nseg = m.nseg; f.flags = (uint32_t*)((char*)ws + y.tail) + 2;
        be.template launch<KXlFold>((int)((f.n + 255) / 256), 256, 0, f, stream);
    }
    // gram of the leading L columns of a panel of `pitch` floats per row: partials to `part`, the matrix to `G`
    void xl_gram_at(const float* pan, int m, int L, int pitch, double* part, double* G) {
        XlGramParams g;
        g.pan = pan; g.m = m; g.L = L; g.pitch = pitch; g.part = part;
        const int nseg = (m + XL_GSEG - 1) / XL_GSEG;
        be.template launch<KXlGram>(nseg * xl_gram_tiles(L), 256, 256 * sizeof(double), g, stream);
        XlGramFoldParams f;
        f.part = g.part; f.G = G; f.L = L; f.nseg = nseg;
        be.template launch<KXlGramFold>((L * L + 255) / 256, 256, 0, f, stream);
    }
    void xl_gram(const float* pan, int m, int L, void* ws, const XlLayout& y) {
        xl_gram_at(pan, m, L, L, (double*)((char*)ws + y.gpart), (double*)((char*)ws + y.G));
    }
    // pan_pitch / out_pitch 0: the panel's rows are L floats, the result's L2 elements apart
    void xl_panel_mm(const float* pan, int m, int L, const float* t, int L2, void* out, int out_dtype, int store_trans,
                     int pan_pitch = 0, int out_pitch = 0, int col0 = 0) {
        XlPanelMmParams q;
        q.pan = pan; q.t = t; q.out = out; q.m = m; q.L = L; q.L2 = L2; q.out_dtype = out_dtype; q.store_trans = store_trans;
        q.pan_pitch = pan_pitch ? pan_pitch : L; q.out_pitch = out_pitch ? out_pitch : L2; q.col0 = col0;
        be.template launch<KXlPanelMm>((int)(((size_t)m * L2 + 255) / 256), 256, 0, q, stream);
    }
    // xl_sym_eig with its host time added to eig_host_us (what tools/tsv_bench.py reads)
    void xl_sym_eig_timed(int n, double* a, double* lam, double* v) {
        const auto t0 = std::chrono::steady_clock::now();
        xl_sym_eig(n, a, lam, v);
        eig_host_us += (unsigned long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t0).count();
    }
    // reads the flags and the Gram back (one synchronisation) and decomposes it; false: the panel or its Gram held a NaN
    // or an Inf (lam and V are then zeros)
    bool xl_eig_readback(int L, void* ws, const XlLayout& y, std::vector<double>& lam, std::vector<double>& V) {
        lam.assign(L, 0.0); V.assign((size_t)L * L, 0.0);
        uint32_t flags[4];
        be.d2h(flags, (char*)ws + y.tail, sizeof flags, stream);
        if (!be.ok()) return true;                              // (reported by the caller as SMHIP_ERR_HIP)
        if (flags[2]) return false;
        std::vector<double> G((size_t)L * L);
        be.d2h(G.data(), (char*)ws + y.G, G.size() * 8, stream);
        if (!be.ok()) return true;
        for (double v : G) if (!geo_finite(v)) return false;
        xl_sym_eig_timed(L, G.data(), lam.data(), V.data());
        return true;
    }
    // Q = orth(Y) (step 6): y_pan -> q_pan, both [m x L]; returns the kept rank, -1: not finite
    int xl_orth(const float* y_pan, float* q_pan, int m, int L, void* ws, const XlLayout& y) {
        xl_gram(y_pan, m, L, ws, y);
        std::vector<double> lam, V;
        if (!xl_eig_readback(L, ws, y, lam, V)) return -1;
        std::vector<float> T((size_t)L * L, 0.f);
        const double cut = geo_dmul(1e-12, lam[0]);
        int kept = 0;
        for (int i = 0; i < L; ++i) {
            if (!(lam[i] > cut)) continue;
            ++kept;
            const double s = geo_dsqrt(lam[i]);
            for (int k = 0; k < L; ++k) T[(size_t)k * L + i] = (float)geo_ddiv(V[(size_t)k * L + i], s);
        }
        float* dT = (float*)((char*)ws + y.T);
        be.h2d(dT, T.data(), T.size() * 4, stream);
        xl_panel_mm(y_pan, m, L, dT, L, q_pan, DT_F32, 0);
        return kept;
    }
    void xl_fill(float* out, int nrows, int L, uint64_t key) {
        XlFillParams f;
        f.out = out; f.n = (size_t)nrows * L; f.key = key;
        be.template launch<KXlFill>((int)(((f.n + 31) / 32 + 255) / 256), 256, 0, f, stream);
    }
    // steps 2 - 4 of smhip_lora_extract, shared with smhip_tsv_merge: from the sketch `omega` [cols x L] (which may be
    // p0) to Q [rows x L] in p0 and C = D^T Q [cols x L] in p1.  The kept rank of each orth goes to orth_rank[n_orth++];
    // false: a panel held a NaN or an Inf
    bool xl_range(const void* ft, const void* base, int dtype, int rows, int cols, int L, int power_iters, const float* omega,
                  float* p0, float* p1, void* ws, const XlLayout& y, int* orth_rank, int& n_orth) {
        auto mm = [&](int trans, const float* x, float* out) { xl_delta_mm(ft, base, dtype, rows, cols, trans, L, x, out, ws, y); };
        mm(0, omega, p1);                                           // Y
        n_orth = 0;
        auto orth = [&](int m) {                                    // p1 -> p0
            const int kept = xl_orth(p1, p0, m, L, ws, y);
            if (kept >= 0) orth_rank[n_orth++] = kept;
            return kept >= 0;
        };
        for (int it = 0; it < power_iters; ++it) {
            if (!orth(rows)) return false;
            mm(1, p0, p1);                                          // Z
            if (!orth(cols)) return false;
            mm(0, p0, p1);                                          // Y
        }
        if (!orth(rows)) return false;                              // Q in p0
        mm(1, p0, p1);                                              // C in p1
        return true;
    }
    int lora_extract(const smhip_extract_desc& d, void* a_out, void* b_out, smhip_extract_report* rep) {
        const XlLayout y = xl_layout(d.rows, d.cols, d.rank);
        const int L = y.L, rows = d.rows, cols = d.cols, r = d.rank;
        *rep = smhip_extract_report{};
        rep->L = L;
        void* ws = d.workspace;
        float* p0 = (float*)ws;
        float* p1 = (float*)((char*)ws + y.pan);
        uint32_t* flags = (uint32_t*)((char*)ws + y.tail);          // [0..1]: the Gram pass's, [2]: xl_fold's
        double* E = (double*)((char*)ws + y.tail + 16);
        be.memset(flags, 0, 32, stream);
        auto nonfinite = [&]() { return fail(SMHIP_ERR_NONFINITE, "lora_extract: NaN or Inf in finetune - base"); };

        // ||D||_F^2: the Gram pass with k = 1 over the layout's segments (there is no out to align: the finetune and the base count)
        TiesInputs in;
        ties_inputs(in, 1, d.in_dtype, (size_t)rows * cols, &d.finetune, &d.base, true);
        gram_pass(in, false, GEO_SEG_ELEMS, y.eseg, (double*)((char*)ws + y.epart), flags, E);

        xl_fill(p0, cols, L, d.key);
        int n_orth = 0;
        if (!xl_range(d.finetune, d.base, d.in_dtype, rows, cols, L, d.power_iters, p0, p0, p1, ws, y, rep->orth_rank, n_orth))
            return nonfinite();
        rep->n_orth = n_orth;
        xl_gram(p1, cols, L, ws, y);
        std::vector<double> lam, V;
        const bool finite = xl_eig_readback(L, ws, y, lam, V);
        if (!be.ok()) return SMHIP_OK;
        if (!finite) return nonfinite();
        const int n = r < L ? r : L;
        const double cut = geo_dmul(1e-12, lam[0]);
        double sum = 0.0;
        int rho = 0;
        for (int i = 0; i < L; ++i) rep->sigma[i] = geo_dsqrt(lam[i] > 0.0 ? lam[i] : 0.0);
        for (int i = 0; i < n; ++i) {
            if (lam[i] > cut) ++rho;
            sum = geo_dadd(sum, lam[i] > 0.0 ? lam[i] : 0.0);
        }
        rep->rho = rho;
        std::vector<float> T((size_t)2 * L * r, 0.f);               // Tb, then Ta, [L x r] each
        for (int i = 0; i < n; ++i) {
            if (!(lam[i] > cut)) continue;
            const double s = geo_dsqrt(rep->sigma[i]);
            for (int k = 0; k < L; ++k) {
                T[(size_t)k * r + i] = (float)geo_dmul(V[(size_t)k * L + i], s);
                T[(size_t)L * r + (size_t)k * r + i] = (float)geo_ddiv(V[(size_t)k * L + i], s);
            }
        }
        float* dT = (float*)((char*)ws + y.T);
        be.h2d(dT, T.data(), T.size() * 4, stream);
        xl_panel_mm(p0, rows, L, dT, r, b_out, d.factor_dtype, 0);
        xl_panel_mm(p1, cols, L, dT + (size_t)L * r, r, a_out, d.factor_dtype, 1);
        double e_host[1];
        uint32_t fl[4];
        be.d2h(e_host, E, 8, stream);
        be.d2h(fl, flags, sizeof fl, stream);                       // the call's last synchronisation
        if (!be.ok()) return SMHIP_OK;
        if (fl[0] || fl[2]) return nonfinite();
        rep->delta_sq = e_host[0];
        rep->share = e_host[0] > 0.0 ? geo_ddiv(sum, e_host[0]) : 0.0;
        return SMHIP_OK;
    }
    // ---- TSV merge (sm_tsv.hpp; smhip_tsv_merge).  The caller's workspace: the extraction's (for L) | Omega [cols x L] |
    // U [rows x Rpm] | W [cols x Rpm] | B [rows x Rpm] | the partials of a Gram of width Rpm | that Gram | M32 [Rpm x Rpm],
    // Rpm = min(256, ceil16(k r)) the widest the panels can get.  U and W have Rpm floats per row whatever Rp is. ----
    struct TsvLayout {
        XlLayout y;
        int r, Rpm;
        size_t omega, U, W, Bp, gpart, G, M, total;
    };
    static TsvLayout tsv_layout(int rows, int cols, int k, int rank) {
        TsvLayout t;
        t.r = std::min(rank, std::min(rows, cols));
        t.y = xl_layout_L(rows, cols, xl_panel_width(rows, cols, t.r), t.r);
        t.Rpm = std::min(TSV_MAX_R, xl_ceil16(k * t.r));
        const size_t mx = (size_t)std::max(rows, cols), Rpm = (size_t)t.Rpm;
        t.omega = t.y.total;
        t.U = t.omega + round_up((size_t)cols * t.y.L * 4, 256);
        t.W = t.U + round_up((size_t)rows * Rpm * 4, 256);
        t.Bp = t.W + round_up((size_t)cols * Rpm * 4, 256);
        t.gpart = t.Bp + round_up((size_t)rows * Rpm * 4, 256);
        t.G = t.gpart + round_up((mx + XL_GSEG - 1) / XL_GSEG * Rpm * Rpm * 8, 256);
        t.M = t.G + round_up(Rpm * Rpm * 8, 256);
        t.total = t.M + round_up(Rpm * Rpm * 4, 256);
        return t;
    }
    void tsv_apply(const float* b, int bp, const float* w, int wp, int rows, int cols, int Rp, const void* base_out, int dtype,
                   double lambda, void* out, float* delta_out) {
        TsvApplyParams a;
        a.b = b; a.w = w; a.rows = rows; a.cols = cols; a.Rp = Rp; a.bp = bp; a.wp = wp;
        a.pvec = (aligned16(b) && aligned16(w) && bp % 4 == 0 && wp % 4 == 0) ? 1 : 0;
        a.base_out = base_out; a.dtype = dtype; a.lambda = (float)lambda; a.out = out; a.delta_out = delta_out;
        a.gn = (cols + TSV_WG - 1) / TSV_WG;
        be.template launch<KTsvApply>((rows + TSV_WG - 1) / TSV_WG * a.gn, 256, 0, a, stream);
    }
    int tsv_merge(const smhip_tsv_desc& d, void* out, float* delta_out, smhip_tsv_report* rep) {
        if (rep) *rep = smhip_tsv_report{};
        if (d.n == 0) return SMHIP_OK;
        const TsvLayout t = tsv_layout(d.rows, d.cols, d.k, d.rank);
        const XlLayout& y = t.y;
        const int L = y.L, rows = d.rows, cols = d.cols, r = t.r, Rpm = t.Rpm;
        char* ws = (char*)d.workspace;
        float* p0 = (float*)ws;
        float* p1 = (float*)(ws + y.pan);
        float* omega = (float*)(ws + t.omega);
        float* U = (float*)(ws + t.U);
        float* W = (float*)(ws + t.W);
        float* Bp = (float*)(ws + t.Bp);
        float* dT = (float*)(ws + y.T);
        uint32_t* flags = (uint32_t*)(ws + y.tail);                 // [0..1]: the Gram pass's, [2]: xl_fold's
        double* E = (double*)(ws + y.tail + 16);                    // delta_sq per finetune
        be.memset(flags, 0, 256, stream);
        be.memset(U, 0, (size_t)rows * Rpm * 4, stream);
        be.memset(W, 0, (size_t)cols * Rpm * 4, stream);
        auto nonfinite = [&](int i) {
            return fail(SMHIP_ERR_NONFINITE, "tsv_merge: NaN or Inf in finetune - base of finetune " + std::to_string(i));
        };
        smhip_tsv_report local;
        smhip_tsv_report& R_ = rep ? *rep : local;
        if (!rep) local = smhip_tsv_report{};
        R_.L = L; R_.r = r;

        xl_fill(omega, cols, L, d.key);
        std::vector<double> s, sums(d.k, 0.0), lam, V;
        int R = 0;
        for (int i = 0; i < d.k; ++i) {
            if (d.alpha[i] == 0.0) continue;
            TiesInputs in;
            ties_inputs(in, 1, d.in_dtype, (size_t)rows * cols, &d.finetune[i], &d.base[i], true);
            gram_pass(in, false, GEO_SEG_ELEMS, y.eseg, (double*)(ws + y.epart), flags, E + i);
            if (!xl_range(d.finetune[i], d.base[i], d.in_dtype, rows, cols, L, d.power_iters, omega, p0, p1, ws, y,
                          R_.orth_rank[i], R_.n_orth[i])) {
                R_.n_orth[i] = 0;
                return nonfinite(i);
            }
            xl_gram(p1, cols, L, ws, y);
            const bool finite = xl_eig_readback(L, ws, y, lam, V);
            if (!be.ok()) return SMHIP_OK;
            if (!finite) return nonfinite(i);
            const double cut = geo_dmul(1e-12, lam[0]);
            int rho = 0;
            for (int j = 0; j < r; ++j) {
                const double l2 = lam[j] > 0.0 ? lam[j] : 0.0;
                R_.sigma[i][j] = geo_dsqrt(l2);
                sums[i] = geo_dadd(sums[i], l2);
                if (lam[j] > cut && rho == j) ++rho;
            }
            R_.rho[i] = rho;
            if (rho) {
                std::vector<float> T((size_t)2 * L * rho);          // V[:, :rho], then V[:, j] / sigma_j, [L x rho] each
                for (int k = 0; k < L; ++k)
                    for (int j = 0; j < rho; ++j) {
                        T[(size_t)k * rho + j] = (float)V[(size_t)k * L + j];
                        T[(size_t)L * rho + (size_t)k * rho + j] = (float)geo_ddiv(V[(size_t)k * L + j], R_.sigma[i][j]);
                    }
                be.h2d(dT, T.data(), T.size() * 4, stream);
                xl_panel_mm(p0, rows, L, dT, rho, U, DT_F32, 0, 0, Rpm, R);
                xl_panel_mm(p1, cols, L, dT + (size_t)L * rho, rho, W, DT_F32, 0, 0, Rpm, R);
            }
            for (int j = 0; j < rho; ++j) s.push_back(geo_dmul(d.alpha[i], R_.sigma[i][j]));
            R += rho;
        }
        const int Rp = xl_ceil16(R);
        R_.R = R; R_.Rp = Rp;

        if (R > 0) {
            // S = sum over the kept j of E_j E_j^T / sqrt(mu_j); 0: fine, else the call's return code
            bool bad = false;
            auto whiten = [&](const float* pan, int m, double* mu_out, int& kept, std::vector<double>& S) {
                xl_gram_at(pan, m, Rp, Rpm, (double*)(ws + t.gpart), (double*)(ws + t.G));
                std::vector<double> G((size_t)Rp * Rp), A((size_t)R * R), mu(R), Ev((size_t)R * R);
                be.d2h(G.data(), ws + t.G, G.size() * 8, stream);
                S.assign((size_t)R * R, 0.0);
                if (!be.ok()) return;
                for (int a = 0; a < R; ++a)
                    for (int b = 0; b < R; ++b) {
                        A[(size_t)a * R + b] = G[(size_t)a * Rp + b];
                        if (!geo_finite(A[(size_t)a * R + b])) bad = true;
                    }
                if (bad) return;
                xl_sym_eig_timed(R, A.data(), mu.data(), Ev.data());
                const double cut = geo_dmul(1e-6, mu[0]);
                for (int j = 0; j < R; ++j) {
                    mu_out[j] = mu[j];
                    if (!(mu[j] > cut)) continue;
                    ++kept;
                    const double sq = geo_dsqrt(mu[j]);
                    for (int a = 0; a < R; ++a) {
                        const double ea = Ev[(size_t)a * R + j];
                        for (int b = 0; b < R; ++b)
                            S[(size_t)a * R + b] = geo_dadd(S[(size_t)a * R + b], geo_ddiv(geo_dmul(ea, Ev[(size_t)b * R + j]), sq));
                    }
                }
            };
            std::vector<double> SU, SW;
            whiten(U, rows, R_.mu_U, R_.kept_U, SU);
            if (!bad) whiten(W, cols, R_.mu_W, R_.kept_W, SW);
            if (!be.ok()) return SMHIP_OK;
            if (bad) return fail(SMHIP_ERR_NONFINITE, "tsv_merge: the singular vectors are not finite");
            std::vector<float> M32((size_t)Rp * Rp, 0.f);
            std::vector<double> row(R);
            for (int a = 0; a < R; ++a) {
                for (int b = 0; b < R; ++b) row[b] = 0.0;
                for (int c = 0; c < R; ++c) {
                    const double us = geo_dmul(SU[(size_t)a * R + c], s[c]);
                    for (int b = 0; b < R; ++b) row[b] = geo_dadd(row[b], geo_dmul(us, SW[(size_t)c * R + b]));
                }
                for (int b = 0; b < R; ++b) M32[(size_t)a * Rp + b] = (float)row[b];
            }
            float* dM = (float*)(ws + t.M);
            be.h2d(dM, M32.data(), M32.size() * 4, stream);
            xl_panel_mm(U, rows, Rp, dM, Rp, Bp, DT_F32, 0, Rpm, Rp, 0);
        }
        tsv_apply(Bp, Rp, W, Rpm, rows, cols, Rp, d.base_out, d.base_out_dtype, d.lambda, out, delta_out);

        double e_host[TIES_MAX_MODELS];
        uint32_t fl[4];
        be.d2h(e_host, E, sizeof e_host, stream);
        be.d2h(fl, flags, sizeof fl, stream);                       // the call's last synchronisation
        if (!be.ok()) return SMHIP_OK;
        if (fl[0] || fl[2]) return fail(SMHIP_ERR_NONFINITE, "tsv_merge: NaN or Inf in finetune - base");
        for (int i = 0; i < d.k; ++i) {
            if (d.alpha[i] == 0.0) continue;
            R_.delta_sq[i] = e_host[i];
            R_.share[i] = e_host[i] > 0.0 ? geo_ddiv(sums[i], e_host[i]) : 0.0;
        }
        return SMHIP_OK;
    }
    int tsv_probe(const float* b, const float* w, int rows, int cols, int Rp, const void* base_out, int dtype, double lambda,
                  void* out, float* delta_out) {
        tsv_apply(b, Rp, w, Rp, rows, cols, Rp, base_out, dtype, lambda, out, delta_out);
        be.sync(stream);
        return SMHIP_OK;
    }

    // ---- Iso-C merge (sm_iso.hpp; smhip_iso_merge).  The caller's workspace: three [rows x cols] fp32 buffers (T oriented,
    // and the two X of the iteration; the second also takes the sum before a transposing copy and Q oriented back) | two
    // [s x s] buffers (G; P) | the partials of the ordered sums | 256 bytes: flags, then the three sums. ----
    struct IsoLayout {
        int s, L;
        size_t n, B1, B2, S1, S2, part, tail, total;
    };
    static IsoLayout iso_layout(int rows, int cols) {
        IsoLayout t;
        t.s = std::min(rows, cols); t.L = std::max(rows, cols);
        t.n = (size_t)rows * cols;
        const size_t nb = round_up(t.n * 4, 256), sb = round_up((size_t)t.s * t.s * 4, 256);
        const size_t nseg = (std::max(t.n, (size_t)t.s * t.s) + GEO_SEG_ELEMS - 1) / GEO_SEG_ELEMS;
        t.B1 = nb; t.B2 = 2 * nb; t.S1 = 3 * nb; t.S2 = t.S1 + sb;
        t.part = t.S2 + sb;
        t.tail = t.part + round_up(nseg * 8, 256);
        t.total = t.tail + 256;
        return t;
    }
    void iso_gemm(int form, int sym, const float* a, int lda, const float* b, int ldb, int M, int N, int K, int ep, float ca,
                  float cb, const float* e, int lde, float* c, int ldc) {
        IsoGemmParams g;
        g.a = a; g.b = b; g.M = M; g.N = N; g.K = K; g.lda = lda; g.ldb = ldb;
        g.avec = (aligned16(a) && lda % 4 == 0) ? 1 : 0; g.bvec = (aligned16(b) && ldb % 4 == 0) ? 1 : 0;
        g.sym = sym; g.ep = ep; g.ca = ca; g.cb = cb; g.e = e; g.lde = lde; g.c = c; g.ldc = ldc;
        const int gm = (M + ISO_WG - 1) / ISO_WG;
        g.gn = (N + ISO_WG - 1) / ISO_WG;
        const int grid = sym ? gm * (gm + 1) / 2 : gm * g.gn;
        if (form == ISO_NT) be.template launch<KIsoGemmNT>(grid, ISO_THREADS, ISO_GEMM_LDS_FLOATS * 4, g, stream);
        else be.template launch<KIsoGemmNN>(grid, ISO_THREADS, ISO_GEMM_LDS_FLOATS * 4, g, stream);
    }
    void iso_transpose(const float* src, float* dst, int rows, int cols) {
        IsoTransposeParams t;
        t.src = src; t.dst = dst; t.rows = rows; t.cols = cols; t.gc = (cols + 31) / 32;
        be.template launch<KIsoTranspose>((rows + 31) / 32 * t.gc, 256, 32 * 33 * 4, t, stream);
    }
    // one ordered fp64 sum: the segments' partials, then their fold into *result (device)
    template <class K>
    void iso_reduce(const float* x, const float* y, size_t n, int s, double* part, double* result) {
        IsoReduceParams r;
        r.x = x; r.y = y; r.n = n; r.s = s; r.part = part;
        const size_t nseg = (n + GEO_SEG_ELEMS - 1) / GEO_SEG_ELEMS;
        be.template launch<K>((int)nseg, GEO_THREADS, iso_reduce_lds_floats() * 4, r, stream);
        fold_pass<KGeoFold>(1, nseg, part, result);
    }
    int iso_merge(const smhip_iso_desc& d, void* out, float* delta_out, smhip_iso_report* rep) {
        smhip_iso_report local;
        smhip_iso_report& R_ = rep ? *rep : local;
        R_ = smhip_iso_report{};
        if (d.n == 0) return SMHIP_OK;
        const IsoLayout t = iso_layout(d.rows, d.cols);
        const int rows = d.rows, cols = d.cols, s = t.s, L = t.L;
        const bool tr = rows > cols;
        char* ws = (char*)d.workspace;
        float* T = (float*)ws;
        float* X = (float*)(ws + t.B1);
        float* Xn = (float*)(ws + t.B2);
        float* G = (float*)(ws + t.S1);
        float* P = (float*)(ws + t.S2);
        double* part = (double*)(ws + t.part);
        uint32_t* flags = (uint32_t*)(ws + t.tail);
        double* res = (double*)(ws + t.tail + 16);                  // [0]: sum X^2, [1]: the residual's sum, [2]: N
        be.memset(flags, 0, 256, stream);
        R_.s = s; R_.L = L; R_.transposed = tr ? 1 : 0;

        // 1, 2: the sum, oriented
        IsoSumParams sp;
        sp.t = tr ? Xn : T;
        ties_inputs(sp.in, d.k, d.in_dtype, d.n, d.finetune, d.base, true);
        for (int i = 0; i < TIES_MAX_MODELS; ++i) sp.alpha[i] = (float)d.alpha[i < d.k ? i : 0];
        sp.flags = flags;
        sp.chunks = pick_chunks((d.n + 7) / 8, 256, 2, 8);
        be.template launch<KIsoSum>(stream_grid((d.n + 7) / 8, 256, sp.chunks), 256, 0, sp, stream);
        if (tr) iso_transpose(Xn, T, rows, cols);
        // 3: the scale
        iso_reduce<KIsoNorm>(T, nullptr, d.n, s, part, res);
        double sum = 0.0;
        uint32_t fl[2];
        be.d2h(fl, flags, sizeof fl, stream);
        be.d2h(&sum, res, 8, stream);
        if (!be.ok()) return SMHIP_OK;
        if (fl[0]) return delta_nonfinite("iso_merge", "finetune - base", d.k, fl[0]);
        const double nu = geo_dsqrt(sum);
        R_.nu = nu;
        if (!geo_finite(nu)) return fail(SMHIP_ERR_NONFINITE, "iso_merge: the sum of the weighted deltas is not finite");
        auto apply = [&](const float* q, float sigma) {
            IsoApplyParams a;
            a.q = q; a.sigma = sigma; a.lambda = (float)d.lambda; a.base_out = d.base_out; a.dtype = d.base_out_dtype;
            a.out = out; a.delta_out = delta_out; a.n = d.n;
            a.aligned = (aligned16(d.base_out) && aligned16(out) && aligned16(delta_out)) ? 1 : 0;
            a.chunks = pick_chunks((d.n + 7) / 8, 256, 2, 8);
            be.template launch<KIsoApply>(stream_grid((d.n + 7) / 8, 256, a.chunks), 256, 0, a, stream);
        };
        if (nu == 0.0) {
            R_.zero = 1;
            be.memset(X, 0, d.n * 4, stream);
            apply(X, 0.f);
            be.sync(stream);
            return SMHIP_OK;
        }
        IsoScaleParams sc;
        sc.x = T; sc.y = X; sc.n = d.n; sc.c = (float)geo_ddiv(1.0, nu);
        be.template launch<KIsoScale>((int)(((d.n + 3) / 4 + 255) / 256), 256, 0, sc, stream);
        // 4: the iteration
        int it = 0;
        bool cubic = false;                                         // the quintic phase is over
        double prev = 0.0;
        for (;; ++it) {
            iso_gemm(ISO_NT, 1, X, L, X, L, s, s, L, ISO_EP_PLAIN, 0.f, 0.f, nullptr, 0, G, s);
            iso_reduce<KIsoResid>(G, nullptr, (size_t)s * s, s, part, res + 1);
            double rs = 0.0;
            be.d2h(&rs, res + 1, 8, stream);                        // the iteration's one synchronisation
            if (!be.ok()) return SMHIP_OK;
            const double e = geo_dsqrt(geo_ddiv(rs, (double)s));
            R_.e[it] = e;
            if (!geo_finite(e)) { R_.iterations = it; return fail(SMHIP_ERR_NONFINITE, "iso_merge: the iteration left the finite numbers"); }
            if (e <= d.tol) { R_.converged = 1; break; }
            if (it == d.max_iter) break;
            if (!(e > ISO_QUINTIC_ABOVE) || (it > 0 && !(e < prev))) cubic = true;
            prev = e;
            if (!cubic) {
                iso_gemm(ISO_NT, 1, G, s, G, s, s, s, s, ISO_EP_POLY, ISO_C5, ISO_B5, G, s, P, s);
                iso_gemm(ISO_NN, 0, P, s, X, L, s, L, s, ISO_EP_AXPY, ISO_A5, 0.f, X, L, Xn, L);
                R_.steps[it] = 'q';
            } else {
                iso_gemm(ISO_NN, 0, G, s, X, L, s, L, s, ISO_EP_CUBIC, ISO_A3, ISO_B3, X, L, Xn, L);
                R_.steps[it] = 'c';
            }
            std::swap(X, Xn);
        }
        R_.iterations = it;
        // 5: the mean singular value
        iso_reduce<KIsoDot>(X, T, d.n, s, part, res + 2);
        double N = 0.0;
        be.d2h(&N, res + 2, 8, stream);
        if (!be.ok()) return SMHIP_OK;
        R_.N = N;
        R_.sigma_bar = geo_ddiv(N, (double)s);
        if (!geo_finite(N)) return fail(SMHIP_ERR_NONFINITE, "iso_merge: the mean singular value is not finite");
        // 6: the output
        if (tr) iso_transpose(X, Xn, cols, rows);
        apply(tr ? Xn : X, (float)R_.sigma_bar);
        be.sync(stream);
        return SMHIP_OK;
    }
    int iso_gemm_probe(const smhip_iso_gemm_desc& d) {
        iso_gemm(d.form, d.sym, d.a, d.lda, d.b, d.ldb, d.M, d.N, d.K, d.epilogue, d.ca, d.cb, d.e, d.lde, d.c, d.ldc);
        be.sync(stream);
        return SMHIP_OK;
    }

    // ---- Delta pack (sm_dpack.hpp; smhip_dpack_pack, smhip_dpack_apply).  bits == 2: the threshold through the shared
    // select path with one finetune (TIES's kernels, unchanged), then in both cases the fused pass, the fold of the rows'
    // partials, the scales (of the rows, or of the one row of the totals), the fold of their terms, ONE readback.
    // Workspace: [the histograms |] DpackHead | the rows' partials [R][5] | the rows' terms [max(R, 1)][2] ----
    struct DpackHead { RadixState state[TIES_MAX_MODELS]; TiesReadback rb; double tot[DPACK_NP]; double T[DPACK_NT]; };
    static int dpack_row_vec(size_t C, const void* a, const void* b) { return (C % 8 == 0 && aligned16(a) && aligned16(b)) ? 1 : 0; }
    int dpack_pack(const smhip_dpack_desc& d, uint8_t* sign, uint8_t* mask, float* scale, smhip_dpack_report* rep) {
        const size_t R = d.rows, C = d.cols, n = R * C, PB = (C + 7) / 8;
        const bool tensor = d.scale_mode == SMHIP_DPACK_TENSOR;
        const unsigned long long k_keep = d.bits == 1 ? (unsigned long long)n : delta_k_keep(d.density, n);
        if (rep) {
            *rep = smhip_dpack_report{};
            rep->rows = R; rep->cols = C; rep->bits = d.bits; rep->k_keep = k_keep;
            rep->threshold = (d.bits == 2 && k_keep == 0) ? INFINITY : 0.f;
        }
        if (n == 0) {                                    // no plane has a byte; the scales are +0
            const size_t ns = tensor ? 1 : R;
            if (ns) be.memset(scale, 0, ns * sizeof(float), stream);
            return SMHIP_OK;
        }
        const size_t part_bytes = round_up(R * DPACK_NP * sizeof(double), 256), terms_bytes = R * DPACK_NT * sizeof(double);
        DpackHead* w;
        size_t off = round_up(sizeof(DpackHead), 256);
        int rc;
        if (d.bits == 2) rc = select_workspace(TIES_MAX_MODELS, w, part_bytes + terms_bytes, &off);
        else rc = plain_workspace(w, off + part_bytes + terms_bytes);
        if (rc) return rc;
        double* part = (double*)ws_at(off);
        double* terms = (double*)ws_at(off + part_bytes);

        if (d.bits == 2) {
            TiesInputs in;
            const void* ft[1] = {d.finetune};
            const void* bs[1] = {d.base};
            ties_inputs(in, 1, d.dtype, n, ft, bs, true);
            ties_thresholds(in, k_keep, w);
        }
        DpackPackParams p;
        p.ft = d.finetune; p.base = d.base; p.dtype = d.dtype;
        p.R = R; p.C = C; p.PB = PB; p.bits = d.bits; p.threshold = w->rb.threshold;
        p.sign = sign; p.mask = mask; p.row_vec = dpack_row_vec(C, d.finetune, d.base);
        p.part = part; p.flags = w->rb.flags;
        be.template launch<KDpackPack>((int)std::min<size_t>(R, (size_t)1 << 20), DPACK_THREADS, dpack_pack_lds_floats() * 4, p, stream);

        fold_pass<KGeoFold>(DPACK_NP, R, part, w->tot);
        DpackScaleParams s;
        s.rows = tensor ? 1 : R; s.part = tensor ? w->tot : part; s.scale = scale; s.terms = terms;
        be.template launch<KDpackScale>((int)((s.rows + 255) / 256), 256, LDS_SCRATCH_FLOATS * 4, s, stream);
        fold_pass<KGeoFold>(DPACK_NT, s.rows, terms, w->T);

        DpackHead host;
        be.d2h(&host, w, sizeof host, stream);           // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;                   // (reported by the caller as SMHIP_ERR_HIP; the report stays as it is)
        if (host.rb.flags[0]) return fail(SMHIP_ERR_NONFINITE, "dpack_pack: NaN or Inf in finetune - base");
        if (rep) {
            if (d.bits == 2) rep->threshold = host.rb.threshold[0];
            rep->kept = (uint64_t)host.tot[3]; rep->nonzero = (uint64_t)host.tot[4];
            rep->resid_sq = host.T[0]; rep->delta_sq = host.T[1];
        }
        return SMHIP_OK;
    }
    int dpack_apply(const smhip_dpack_apply_desc& d, void* out) {
        const size_t R = d.rows, C = d.cols, PB = (C + 7) / 8;
        if (R * C == 0) return SMHIP_OK;
        DpackApplyParams p;
        p.base = d.base; p.dtype = d.dtype; p.R = R; p.C = C; p.PB = PB; p.units = R * PB;
        p.sign = d.sign; p.mask = d.mask; p.scale = d.scale; p.scale_mode = d.scale_mode == SMHIP_DPACK_TENSOR ? DPACK_TENSOR : DPACK_ROW;
        p.out = out; p.row_vec = dpack_row_vec(C, d.base, out);
        p.chunks = pick_chunks(p.units, 256, 2, 8);
        be.template launch<KDpackApply>(stream_grid(p.units, 256, p.chunks), 256, LDS_SCRATCH_FLOATS * 4, p, stream);
        return SMHIP_OK;
    }

    // ---- EMR-Merging (sm_emr.hpp; smhip_emr_merge, smhip_emr_mask, smhip_emr_apply).  The unified model: no select, one
    // kernel, the workspace is EmrReadback alone.  A task's mask: the fused pass over whole rows, the fold of the rows'
    // partials, ONE readback; the rescaler and the residual are formed here from the seven totals.
    // Workspace of the mask: EmrMaskHead | the rows' partials [R][7] ----
    struct EmrReadback {
        unsigned long long agree[TIES_MAX_MODELS], winner[TIES_MAX_MODELS], counts[EMR_COUNTS];
        uint32_t flags[2];
    };
    int emr_merge(const smhip_emr_desc& d, void* out, float* delta_out, smhip_emr_report* rep) {
        const int k = d.k;
        if (rep) {
            *rep = smhip_emr_report{};
            rep->n = d.n;
        }
        if (d.n == 0) return SMHIP_OK;
        EmrReadback* w;
        int rc;
        if ((rc = plain_workspace(w))) return rc;

        EmrMergeParams m;
        delta_inputs(d, out, delta_out, false, m);
        m.lambda = (float)d.lambda;
        m.agree = w->agree; m.winner = w->winner; m.counts = w->counts; m.flags = w->flags;
        const int grid = stream_grid((d.n + 7) / 8, 256, m.chunks);
        const size_t lds = (LDS_SCRATCH_FLOATS + emr_lds_words(k, 256)) * 4;
        if (k <= EMR_REG_SMALL) be.template launch<KEmrMerge>(grid, 256, lds, m, stream);
        else be.template launch<KEmrMergeAny>(grid, 256, lds, m, stream);

        EmrReadback host;
        if ((rc = delta_readback("emr_merge", k, w, host))) return rc;     // the call's one synchronisation
        if (host.flags[1]) return fail(SMHIP_ERR_NONFINITE, "emr_merge: NaN or Inf in the sum of the deltas");
        if (rep) {
            for (int i = 0; i < k; ++i) { rep->agree[i] = host.agree[i]; rep->winner[i] = host.winner[i]; }
            rep->elected_pos = host.counts[EMR_POS]; rep->elected_neg = host.counts[EMR_NEG];
            rep->zero = host.counts[EMR_ZERO]; rep->contested = host.counts[EMR_CONTESTED];
        }
        return SMHIP_OK;
    }
    struct EmrMaskHead { double tot[EMR_NP]; uint32_t flags[2]; };
    static int emr_row_vec(size_t C, const void* a, const void* b, const void* c) {
        return (C % 8 == 0 && aligned16(a) && aligned16(b) && aligned16(c)) ? 1 : 0;
    }
    int emr_mask(const smhip_emr_mask_desc& d, uint8_t* mask, float* scale, smhip_emr_mask_report* rep) {
        const size_t R = d.rows, C = d.cols, n = R * C, PB = (C + 7) / 8;
        if (rep) {
            *rep = smhip_emr_mask_report{};
            rep->rows = R; rep->cols = C;
        }
        if (n == 0) {                                    // the plane has no byte; the rescaler is +0
            be.memset(scale, 0, sizeof(float), stream);
            return SMHIP_OK;
        }
        EmrMaskHead* w;
        const size_t off = round_up(sizeof(EmrMaskHead), 256);
        int rc;
        if ((rc = plain_workspace(w, off + R * EMR_NP * sizeof(double)))) return rc;
        double* part = (double*)ws_at(off);

        EmrMaskParams p;
        p.ft = d.finetune; p.base = d.base; p.uni = d.unified; p.dtype = d.dtype;
        p.R = R; p.C = C; p.PB = PB; p.mask = mask; p.row_vec = emr_row_vec(C, d.finetune, d.base, d.unified);
        p.part = part; p.flags = w->flags;
        be.template launch<KEmrMask>((int)std::min<size_t>(R, (size_t)1 << 20), EMR_THREADS, emr_mask_lds_floats() * 4, p, stream);
        fold_pass<KGeoFold>(EMR_NP, R, part, w->tot);

        EmrMaskHead host;
        be.d2h(&host, w, sizeof host, stream);           // the call's one synchronisation
        if (!be.ok()) return SMHIP_OK;                   // (reported by the caller as SMHIP_ERR_HIP; the report stays as it is)
        if (host.flags[0] & 1u) return fail(SMHIP_ERR_NONFINITE, "emr_mask: NaN or Inf in finetune - base");
        if (host.flags[0] & 2u) return fail(SMHIP_ERR_NONFINITE, "emr_mask: NaN or Inf in unified - base");
        const float l = emr_scale_of(host.tot[0], host.tot[1]);
        be.h2d(scale, &l, sizeof l, stream);
        if (rep) {
            rep->A = host.tot[0]; rep->B = host.tot[1]; rep->D2 = host.tot[2]; rep->X = host.tot[3]; rep->U2 = host.tot[4];
            rep->c = (uint64_t)host.tot[5]; rep->nonzero = (uint64_t)host.tot[6];
            rep->lambda = l; rep->delta_sq = host.tot[2]; rep->resid_sq = emr_resid_of(host.tot[2], host.tot[3], host.tot[4], l);
        }
        return SMHIP_OK;
    }
    // The unified model and every task's modulator from one call (sm_emr_fused.hpp; smhip_emr_merge_masks): the fused
    // pass over whole rows, ONE fold of the rows' 7k partials, ONE readback of the counters, the flags and the 7k
    // totals; the k rescalers are formed here and copied to the device.  Workspace: EmrFusedHead | part [R][k][7] ----
    struct EmrFusedHead {
        unsigned long long agree[TIES_MAX_MODELS], winner[TIES_MAX_MODELS], counts[EMR_COUNTS];
        uint32_t flags[4];
        double tot[TIES_MAX_MODELS * EMR_NP];
    };
    bool emr_fused_geo_fold = false;          // test and bench hook "emr_fused_geo_fold": fold with geo_gram_fold (the same bits)
    int emr_merge_masks(const smhip_emr_desc& d, size_t R, size_t C, void* out, float* delta_out, uint8_t* const* masks,
                        float* const* scales, smhip_emr_report* rep, smhip_emr_mask_report* mreps) {
        const int k = d.k;
        if (rep) {
            *rep = smhip_emr_report{};
            rep->n = d.n;
        }
        for (int i = 0; mreps && i < k; ++i) {
            mreps[i] = smhip_emr_mask_report{};
            mreps[i].rows = R; mreps[i].cols = C;
        }
        if (d.n == 0) {                                  // the planes have no byte; the rescalers are +0
            for (int i = 0; i < k; ++i) be.memset(scales[i], 0, sizeof(float), stream);
            return SMHIP_OK;
        }
        EmrFusedHead* w;
        const size_t off = round_up(sizeof(EmrFusedHead), 256);
        int rc;
        if ((rc = plain_workspace(w, off + R * k * EMR_NP * sizeof(double)))) return rc;
        double* part = (double*)ws_at(off);

        EmrFusedParams m;
        ties_inputs(m.in, k, d.in_dtype, d.n, d.finetune, d.base, aligned16(out) && aligned16(delta_out) && aligned16(d.base_out));
        m.base_out = d.base_out; m.base_out_dtype = d.base_out_dtype;
        m.out_is_base0 = (m.in.shared_base && d.base_out == m.in.base[0] && d.base_out_dtype == d.in_dtype) ? 1 : 0;
        m.lambda = (float)d.lambda; m.out = out; m.delta_out = delta_out;
        m.agree = w->agree; m.winner = w->winner; m.counts = w->counts; m.flags = w->flags;
        m.R = R; m.C = C; m.PB = (C + 7) / 8; m.row_vec = (m.in.aligned && C % 8 == 0) ? 1 : 0;
        for (int i = 0; i < TIES_MAX_MODELS; ++i) m.mask[i] = masks[i < k ? i : 0];
        m.part = part;
        const int grid = (int)std::min<size_t>(R, (size_t)1 << 20);
        if (k <= EMR_REG_SMALL) be.template launch<KEmrMergeMask>(grid, EMR_THREADS, emr_fused_lds_bytes(k, EMR_THREADS), m, stream);
        else be.template launch<KEmrMergeMaskAny>(grid, EMR_THREADS, emr_fused_lds_bytes(k, EMR_THREADS), m, stream);
        if (emr_fused_geo_fold) {
            fold_pass<KGeoFold>(EMR_NP * k, R, part, w->tot);
        } else {
            EmrFoldParams f;
            f.np = EMR_NP * k; f.nseg = R; f.part = part; f.out = w->tot;
            be.template launch<KEmrFold>(1, EMR_FOLD_THREADS, emr_fold_lds_bytes(f.np), f, stream);
        }

        EmrFusedHead host;
        if ((rc = delta_readback("emr_merge_masks", k, w, host))) {      // the call's one synchronisation
            uint32_t lowest = host.flags[0] & (0u - host.flags[0]);      // (the message names the lowest such finetune)
            return delta_nonfinite("emr_merge_masks", "finetune - base", k, lowest);
        }
        if (!be.ok()) return SMHIP_OK;                   // (reported by the caller as SMHIP_ERR_HIP; the reports stay as they are)
        if (host.flags[1]) return fail(SMHIP_ERR_NONFINITE, "emr_merge_masks: NaN or Inf in the sum of the deltas");
        if (host.flags[2]) {
            int i = 0;
            while (!(host.flags[2] & (1u << i))) ++i;
            return fail(SMHIP_ERR_NONFINITE, "emr_merge_masks: NaN or Inf in unified - base of entry " + std::to_string(i));
        }
        if (rep) {
            for (int i = 0; i < k; ++i) { rep->agree[i] = host.agree[i]; rep->winner[i] = host.winner[i]; }
            rep->elected_pos = host.counts[EMR_POS]; rep->elected_neg = host.counts[EMR_NEG];
            rep->zero = host.counts[EMR_ZERO]; rep->contested = host.counts[EMR_CONTESTED];
        }
        float ls[TIES_MAX_MODELS];
        bool run = true;                                 // the k rescalers stand one after the other: one copy
        for (int i = 0; i < k; ++i) {
            ls[i] = emr_scale_of(host.tot[(size_t)i * EMR_NP], host.tot[(size_t)i * EMR_NP + 1]);
            run = run && scales[i] == scales[0] + i;
        }
        if (run) be.h2d(scales[0], ls, k * sizeof(float), stream);
        for (int i = 0; i < k; ++i) {
            const double* t = host.tot + (size_t)i * EMR_NP;
            const float l = ls[i];
            if (!run) be.h2d(scales[i], &l, sizeof l, stream);
            if (mreps) {
                smhip_emr_mask_report& q = mreps[i];
                q.A = t[0]; q.B = t[1]; q.D2 = t[2]; q.X = t[3]; q.U2 = t[4];
                q.c = (uint64_t)t[5]; q.nonzero = (uint64_t)t[6];
                q.lambda = l; q.delta_sq = t[2]; q.resid_sq = emr_resid_of(t[2], t[3], t[4], l);
            }
        }
        return SMHIP_OK;
    }
    int emr_apply(const smhip_emr_apply_desc& d, void* out) {
        const size_t R = d.rows, C = d.cols, PB = (C + 7) / 8;
        if (R * C == 0) return SMHIP_OK;
        EmrApplyParams p;
        p.base = d.base; p.uni = d.unified; p.dtype = d.dtype; p.R = R; p.C = C; p.PB = PB; p.units = R * PB;
        p.mask = d.mask; p.scale = d.scale;
        p.out = out; p.row_vec = emr_row_vec(C, d.base, d.unified, out);
        p.chunks = pick_chunks(p.units, 256, 2, 8);
        be.template launch<KEmrApply>(stream_grid(p.units, 256, p.chunks), 256, LDS_SCRATCH_FLOATS * 4, p, stream);
        return SMHIP_OK;
    }

    int xl_probe(const smhip_xl_probe_desc& d) {
        const int L = d.L;
        if (d.op == SMHIP_XL_SYM_EIG) {
            std::vector<double> a((const double*)d.x, (const double*)d.x + (size_t)L * L);
            xl_sym_eig(L, a.data(), (double*)d.y, (double*)d.y + L);
            return SMHIP_OK;
        }
        if (d.op == SMHIP_XL_FILL) {
            XlFillParams f;
            f.out = (float*)d.y; f.n = (size_t)d.rows * L; f.key = d.key;
            be.template launch<KXlFill>((int)(((f.n + 31) / 32 + 255) / 256), 256, 0, f, stream);
            return SMHIP_OK;
        }
        if (d.op == SMHIP_XL_PANEL_MM) {
            xl_panel_mm((const float*)d.x, d.rows, L, d.t, d.L2, d.y, d.out_dtype, d.trans);
            return SMHIP_OK;
        }
        const XlLayout y = xl_layout_L(d.rows, d.cols, L, L);
        if (!d.workspace || d.workspace_bytes < y.total) return fail(SMHIP_ERR_ARG, "xl_probe: the workspace is too small");
        if (d.op == SMHIP_XL_GRAM) {
            xl_gram((const float*)d.x, d.rows, L, d.workspace, y);
            std::vector<double> G((size_t)L * L);
            be.d2h(G.data(), (char*)d.workspace + y.G, G.size() * 8, stream);
            be.h2d(d.y, G.data(), G.size() * 8, stream);
            return SMHIP_OK;
        }
        be.memset((char*)d.workspace + y.tail, 0, 32, stream);
        xl_delta_mm(d.finetune, d.base, d.in_dtype, d.rows, d.cols, d.trans, L, (const float*)d.x, (float*)d.y, d.workspace, y);
        be.sync(stream);
        return SMHIP_OK;
    }

  private:
    Buffer ws_;      // the operators' workspace: selection histograms, states, partials, row data, the readback
};

}  // namespace smhip
