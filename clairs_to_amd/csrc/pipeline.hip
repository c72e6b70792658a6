// Native chunk pipeline: candidate chunk files + pileup source (mpileup text or BAM) -> p_<chunk>.vcf, the whole of what
// pileup_call.prepare_chunk / launch_chunk / finish_chunk do per chunk, as one C call (cto_run_chunks).
//
//   producers (N threads)  BED -> centres, reference slice (.fai), column pack (tokeniser / BAM reader; for some BAM chunks with the
//                          BGZF blocks inflated on the device, InflateCtx), one upload out of a page-locked staging buffer on the
//                          producer's own stream into the device buffers of a free slot
//   launcher (the caller)  waits for the upload event; featurisation, both networks, posterior; the candidates' column vectors
//                          gathered on the device; one copy of everything the writers need on the copy-back stream; an event
//   writers (M threads)    alt_info strings + every VCF record (two C calls), file write; the slot goes back to the pool
//
// The Python pipeline (call_chunks.run_pipeline) runs the same stages with the same C calls on thread pools.  Moving the loop here did
// not by itself change the rate (the interpreter was not the bound); what did was what the loop can own once it is native: the
// staging buffers the tokeniser merges into, buffers and contexts kept from chunk to chunk and from call to call, waits that sleep
// instead of spinning, CU-masked streams for the device inflate (DESIGN.md section 6 has the sequence of measurements).
// Outputs are byte-identical (tests/test_gpu_cli.py).
//
// Here: the two layouts every stage shares (PackLayout, ResultLayout), a chunk's Slot, Run - the state of one call with the producers'
// half (produce), the launcher's (launch / launch_stream) and the writers' (finish) - and run_chunks, which sets a call up.  What needs
// no GPU (files, .fai, BED intervals, the child process, the queue, the clocks) is run_files.h; owning handles are hip_buffers.h.
#include <unistd.h>

#include <algorithm>
#include <atomic>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "bam_span.h"
#include "common.h"
#include "hip_buffers.h"
#include "inflated_span.h"
#include "pack_internal.h"
#include "run_files.h"

using namespace cto;
using namespace cto::run_files;

namespace {

// What the writers need of a chunk, in ONE device buffer that comes back with ONE copy:
// site_info | candidate column vectors | sitefirst | decision | qual | keycnt | keyfirst, each part 256-byte aligned.
struct ResultLayout {
    static constexpr size_t SITE_INFO_ROW = 48, COLVEC_ROW = CTO_COLVEC_STRIDE * 2, SITEFIRST_ROW = 32, DECISION_ROW = 16, QUAL_ROW = 8,   // per site
                            KEYCNT_ROW = 4, KEYFIRST_ROW = 8;                                                                               // per key
    enum { SITE_INFO, COLVEC, SITEFIRST, DECISION, QUAL, KEYCNT, KEYFIRST, PARTS };
    size_t off[PARTS] = {0, 0, 0, 0, 0, 0, 0}, total = 0;
    ResultLayout() = default;
    ResultLayout(int64_t n_sites, int64_t n_keys) {
        const size_t n = size_t(n_sites), nk = size_t(std::max<int64_t>(n_keys, 1));
        const size_t bytes[PARTS] = {n * SITE_INFO_ROW, n * COLVEC_ROW, n * SITEFIRST_ROW, n * DECISION_ROW, n * QUAL_ROW, nk * KEYCNT_ROW, nk * KEYFIRST_ROW};
        for (int i = 0; i < PARTS; ++i) { off[i] = total; total += (bytes[i] + 255) / 256 * 256; }
    }
    // the parts behind `base`: the slot's device buffer or its page-locked copy
    template <class T> T* part(void* base, int i) const { return reinterpret_cast<T*>(static_cast<char*>(base) + off[i]); }
    int32_t* site_info(void* base) const { return part<int32_t>(base, SITE_INFO); }
    int16_t* colvec(void* base) const { return part<int16_t>(base, COLVEC); }
    int32_t* sitefirst(void* base) const { return part<int32_t>(base, SITEFIRST); }
    int32_t* decision(void* base) const { return part<int32_t>(base, DECISION); }
    double* qual(void* base) const { return part<double>(base, QUAL); }
    uint32_t* keycnt(void* base) const { return part<uint32_t>(base, KEYCNT); }
    int32_t* keyfirst(void* base) const { return part<int32_t>(base, KEYFIRST); }
};

struct Slot {
    // pack on the device
    DevBuf pack_dev;                     // the pack arrays + the candidate positions, one allocation (PackLayout)
    PinBuf stage;                        // its page-locked source
    const int32_t* d_site_pos = nullptr;
    // featurisation / network / epilogue outputs
    DevBuf colvec, coldepth, x_aff, x_neg, la, ln, post;
    DevBuf dec_l, qual_l;                // decision / QUAL of one network launch, before they are dealt out to the chunks they belong to
    DevBuf xflags, xdepth, xscratch, cand, cand_scr;    // REGION jobs: candidate gates' outputs, overflow counters, candidate positions (+ count)
    PinBuf cand_host;
    DevBuf xmode;                        // REGION jobs with a confident BED / an indel BED / a hybrid list: intervals, positions, hybrid_info records
    PinBuf xmode_host;
    DevBuf res_dev;                      // the chunk's results (ResultLayout)
    PinBuf res_host;                     // the same bytes on the host, one copy per chunk
    ResultLayout res;                    // of the chunk in the slot, set when it is launched
    Event uploaded, begin, computed, done, kernels_end;
    // host side of the chunk
    int64_t job = -1;
    int device = 0;
    cto_pack* pack = nullptr;
    cto_pack_view hv{}, dv{};
    std::vector<int32_t> sites;
    std::string ref;
    int64_t ref_start = 0;
    cto_dev_tokeniser* tok = nullptr;    // text input with cfg.device_tokenise: the slot's tokeniser context (text staging + row tables)
    int open(int dev) {
        device = dev;
        int rc;
        if ((rc = uploaded.create(hipEventDisableTiming)) || (rc = begin.create()) || (rc = computed.create(hipEventDisableTiming)) ||
            (rc = kernels_end.create()) || (rc = done.create(hipEventBlockingSync)))      // writers sleep, not spin, until their chunk is back
            return rc;
        return CTO_OK;
    }
    void drop_pack() { if (pack) { cto_pack_free(pack); pack = nullptr; } }
    ~Slot() { if (tok) cto_dev_tokeniser_destroy(tok); drop_pack(); }
};

// One chunk's trip through the device inflate (csrc/inflate.hip): the BGZF byte range, its block table and the inflated blocks
// (InflatedSpan), the inflated blocks on the host for the host reader, and a stream CONFINED to the first `cus` compute units
// (hipExtStreamCreateWithCUMask; tools/cumask_probe.hip: N leading bits = N / 8 CUs of every XCD).  A wave-per-block inflate launch
// occupies its CUs for tens of milliseconds; unconfined, the networks' block kernels - which need a CU's whole register file -
// wait for those waves to drain, confined they run on the other CUs.
struct InflateCtx {
    cto_dev_pileup* pile = nullptr;      // reads -> columns on the device (csrc/pileup.hip), created on first use
    int device = 0, cus = 0;
    InflatedSpan span;
    PinBuf h_out, h_sites;               // h_out: the inflated span back on the host (the host reader piles it up); h_sites: the chunk's
                                         // candidate positions on their way up (page-locked like every copy source)
    Stream stream;                       // (after the buffers: drained before they are freed)
    Event landed;                        // recorded behind the copy back; the producer thread sleeps on it (wait_event)
    int open(int dev, int n_cus) {
        device = dev; cus = n_cus;
        uint32_t mask[8] = {0, 0, 0, 0, 0, 0, 0, 0};
        for (int i = 0; i < n_cus && i < 256; ++i) mask[i / 32] |= 1u << (i % 32);
        const int rc = stream.create_on_cus(mask, 8);
        return rc != CTO_OK ? rc : landed.create(hipEventBlockingSync | hipEventDisableTiming);
    }
    ~InflateCtx() { if (pile) cto_dev_pileup_destroy(pile); }
};

__global__ void k_gather_rows(const int16_t* __restrict__ colvec, const int32_t* __restrict__ site_info, int64_t n, int16_t* __restrict__ out) {
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const int32_t c = site_info[i * 12];
    const int64_t col = c < 0 ? 0 : c;
    if (threadIdx.x < CTO_COLVEC_STRIDE) out[i * CTO_COLVEC_STRIDE + threadIdx.x] = colvec[col * CTO_COLVEC_STRIDE + threadIdx.x];
}

// Slots (device + page-locked buffers, events) and device-inflate contexts outlive the call: allocating and freeing ~100 MB of them
// per slot costs tens of milliseconds, which a short chunk list would pay on every call; cto_run_release() frees them.
// never destroyed: at process exit the HIP runtime may already be gone when static destructors run
std::mutex& slot_cache_m() { static std::mutex* m = new std::mutex(); return *m; }
std::vector<std::unique_ptr<Slot>>& slot_cache() { static auto* v = new std::vector<std::unique_ptr<Slot>>(); return *v; }
std::vector<std::unique_ptr<InflateCtx>>& inflate_cache() { static auto* v = new std::vector<std::unique_ptr<InflateCtx>>(); return *v; }

// A call's share of a cache: up to `want` entries that `fits` move out of it; however the call ends, all of its own go (back) in
template <class T>
struct Lease {
    std::vector<std::unique_ptr<T>>& cache;
    std::vector<std::unique_ptr<T>>* mine;
    void (*before_return)(T&);               // what an entry lets go of first (may be null)
    template <class Fits>
    void take(int want, Fits fits) {
        std::lock_guard<std::mutex> g(slot_cache_m());
        for (size_t i = 0; i < cache.size() && int(mine->size()) < want;)
            if (fits(*cache[i])) { mine->push_back(std::move(cache[i])); cache.erase(cache.begin() + long(i)); }
            else ++i;
    }
    ~Lease() {
        std::lock_guard<std::mutex> g(slot_cache_m());
        for (auto& x : *mine) { if (before_return) before_return(*x); cache.push_back(std::move(x)); }
        mine->clear();
    }
};

constexpr int FLANK_POS = 33, EXPAND_REF = 1000;       // shared/param.py no_of_positions, expand_reference_region
constexpr int REGION_FLANK = 17;                       // flankingBaseNum + 1: the window columns of a candidate at the edge of a region

// A pack in a slot's device buffer: its seven arrays + the chunk's candidate positions in ONE allocation, each part 256-byte aligned
// with 256 bytes behind it.  The page-locked staging buffer of the upload path has the same layout.
struct PackLayout : UploadParts {        // src: the arrays of `v` (host or device) and the site list
    enum { SITES = 7, PARTS = 8 };
    PackLayout(const cto_pack_view& v, const void* sites, size_t n_sites) {
        const size_t nc = size_t(v.n_cols), ne = size_t(v.n_entries), nk = size_t(v.n_keys);
        const void* s[PARTS] = {v.entries, v.col_pos, v.col_ref, v.col_off, v.key_off, v.key_meta, v.key_group, sites};
        const size_t b[PARTS] = {ne * 4, nc * 4, nc, (nc + 1) * 8, (nc + 1) * 4, nk, nk * 4, n_sites * 4};
        for (int i = 0; i < PARTS; ++i) add(s[i], b[i]);
    }
    // the pointers of `v` (its counts are the caller's) and the site list, in the allocation at `base`
    void bind(void* base, cto_pack_view* v, const int32_t** d_site_pos) const {
        v->entries = at<uint32_t>(base, 0);
        v->col_pos = at<int32_t>(base, 1);
        v->col_ref = at<uint8_t>(base, 2);
        v->col_off = at<int64_t>(base, 3);
        v->key_off = at<int32_t>(base, 4);
        v->key_meta = at<uint8_t>(base, 5);
        v->key_group = at<int32_t>(base, 6);
        *d_site_pos = at<int32_t>(base, SITES);
    }
};

// A pack born on the device (pile-up, tokeniser) becomes the slot's: its arrays `dvw` move from the context that made them into the slot's
// one device allocation, laid out as the upload path lays it out, + the candidate positions out of `site_stage`; `lite` is the host's part.
// s->uploaded is recorded; `wait_on` (that event, or one recorded right behind it) is waited for: context and `site_stage` are free again.
int adopt_device_pack(Slot* s, const cto_pack_view& dvw, cto_pack* lite, PinBuf& site_stage, hipStream_t stream, hipEvent_t wait_on) {
    const size_t ns = s->sites.size();
    int rc = site_stage.ensure(ns * 4 + 256);
    const PackLayout lay(dvw, site_stage.p, ns);
    if (rc != CTO_OK || (rc = s->pack_dev.ensure(lay.total)) != CTO_OK) { cto_pack_free(lite); return rc; }
    memcpy(site_stage.p, s->sites.data(), ns * 4);
    char* d = static_cast<char*>(s->pack_dev.p);
    for (int i = 0; i < PackLayout::PARTS; ++i)
        if (lay.bytes[i])
            CTO_HIP(hipMemcpyAsync(d + lay.off[i], lay.src[i], lay.bytes[i], i == PackLayout::SITES ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice, stream));
    if (s->pack) cto_pack_free(s->pack);
    s->pack = lite;
    s->hv = cto_pack_view{};
    s->hv.n_cols = dvw.n_cols; s->hv.n_entries = dvw.n_entries; s->hv.n_keys = dvw.n_keys;
    s->dv = s->hv;
    lay.bind(d, &s->dv, &s->d_site_pos);
    CTO_HIP(hipEventRecord(s->uploaded, stream));
    if (wait_on != s->uploaded.e) CTO_HIP(hipEventRecord(wait_on, stream));
    CTO_HIP(wait_event(wait_on));
    return CTO_OK;
}

struct Run {
    const cto_run_cfg* cfg;
    const cto_chunk_job* jobs;
    int64_t n_jobs;
    std::atomic<int64_t> next_job{0};
    std::vector<std::unique_ptr<Slot>> slots;
    Queue<Slot*> free_slots, to_launch, to_write;
    std::mutex err_m;
    std::string first_error;
    std::atomic<bool> failed{false};
    std::atomic<int64_t> candidates{0}, sites{0}, rows{0}, low_cov{0}, clamped{0};
    std::mutex stat_m;
    cto_run_stats st{};                  // its times (under stat_m, the launcher's are its own); the counters are added at the end
    Mapped fasta;
    std::vector<std::unique_ptr<InflateCtx>> inflate_ctx;
    Queue<InflateCtx*> free_ctx;
    std::atomic<int64_t> device_inflated{0}, device_piled{0}, device_tokenised{0};
    std::mutex fai_m;
    std::map<std::string, FaiRec> fai;
    // --call_indels_only_in_these_regions: per contig the rows as sorted, merged [begin, end) intervals (run_files.h load_indel_regions)
    std::map<std::string, std::vector<int64_t>> indel_regions;
    bool fai_of(const std::string& ctg, FaiRec* rec, std::string* err) {
        std::lock_guard<std::mutex> g(fai_m);
        auto it = fai.find(ctg);
        if (it != fai.end()) { *rec = it->second; return true; }
        if (!fai_lookup(cfg->ref_fa, ctg, rec, err)) return false;
        fai[ctg] = *rec;
        return true;
    }

    void fail(const std::string& msg) {
        std::lock_guard<std::mutex> g(err_m);
        if (first_error.empty()) first_error = msg;
        failed = true;
    }

    // cto_pack_from_bam with the chunk's BGZF blocks inflated on the device (the sequence of include/clairsto_amd.h: chunk span ->
    // scan -> inflate -> pile-up from memory).  *done = 0 with CTO_OK: nothing to send (no whole block in the span) - the caller reads
    // the chunk on the host.
    int pack_from_bam_device(const cto_chunk_job& j, const std::string& ctg, int64_t lo, int64_t hi, const std::vector<int64_t>& iv, Slot* s,
                             InflateCtx* c, int* done) {
        const bool timing = getenv("CTO_PIPE_TIMING") != nullptr;
        const double T0 = now_s(), C0 = cpu_s();
        int64_t fb = 0, fe = 0;
        int rc = cto_bam_chunk_span(j.bam_path, nullptr, ctg.c_str(), lo, hi, &fb, &fe);
        if (rc != CTO_OK) return rc;
        const size_t nbytes = fe > fb ? size_t(fe - fb) : 0;
        if (nbytes == 0) return CTO_OK;
        const double Cs = cpu_s();
        InflatedSpan& sp = c->span;
        if ((rc = sp.read(j.bam_path, fb, nbytes, "")) != CTO_OK) return rc;
        const double T1 = now_s(), C1 = cpu_s();
        const int64_t n = sp.scan();
        if (n < 0) return int(n);
        if (n == 0) return CTO_OK;
        const cto_bgzf_block* blocks = sp.blocks();
        const auto all_inflated = [&]() -> int {      // the blocks' status words, once they are back
            const int64_t b = sp.first_bad_status();
            CTO_REQUIRE(b < 0, CTO_EINVAL, "%s: the BGZF block at file offset %llu does not inflate (status %d)", j.bam_path,
                        (unsigned long long)blocks[b].file_off, sp.h_status.as<int>()[b]);
            return CTO_OK;
        };
        const double T2 = now_s(), C2 = cpu_s();
        if ((rc = sp.inflate(c->stream))) return rc;      // the blocks' status words are on their way back behind it
        if (cfg->device_pileup) {
            // reads -> columns on the device: only the status words come back before the pile-up
            CTO_HIP(hipEventRecord(c->landed, c->stream));
            CTO_HIP(wait_event(c->landed));
            if ((rc = all_inflated()) != CTO_OK) return rc;
            if (!c->pile && (rc = cto_dev_pileup_create(&c->pile))) return rc;
            std::vector<uint64_t> voffs;
            int32_t tid = -1;
            const int64_t n_st = record_starts(j.bam_path, nullptr, ctg.c_str(), lo, hi, fb, fe, &voffs, &tid);
            if (n_st < 0 && n_st != CTO_ENOMEM) return int(n_st);
            int fallback = n_st <= 0;                                               // still too many: the host reader takes the chunk
            cto_pack_view dvw{};
            cto_pack* lite = nullptr;
            if (!fallback) {
                rc = cto_pileup_device(c->pile, sp.d_out.p, blocks, n, voffs.data(), n_st, tid, lo, hi, iv.empty() ? nullptr : iv.data(), int64_t(iv.size() / 2),
                                       s->ref.data(), s->ref_start, s->ref.size(), 2316, 0, cfg->max_depth, cfg->max_indel_length, c->stream, &dvw, &lite, &fallback);
                if (rc != CTO_OK) return rc;
            }
            if (!fallback) {
                if ((rc = adopt_device_pack(s, dvw, lite, c->h_sites, c->stream, c->landed)) != CTO_OK) return rc;
                if (timing)
                    fprintf(stderr, "device pile-up: %.1f MB in %lld blocks -> %lld columns, %lld entries: read %.1f ms, inflate + pile-up %.1f; thread CPU: span %.1f ms, read %.1f, scan %.1f, rest %.1f\n", nbytes / 1e6,
                            (long long)n, (long long)dvw.n_cols, (long long)dvw.n_entries, (T1 - T0) * 1e3, (now_s() - T2) * 1e3, (Cs - C0) * 1e3, (C1 - Cs) * 1e3, (C2 - C1) * 1e3, (cpu_s() - C2) * 1e3);
                *done = 2;
                ++device_inflated;
                ++device_piled;
                return CTO_OK;
            }
        }
        if ((rc = c->h_out.ensure(sp.out_al))) return rc;
        CTO_HIP(hipMemcpyAsync(c->h_out.p, sp.d_out.p, sp.out_al, hipMemcpyDeviceToHost, c->stream));
        CTO_HIP(hipEventRecord(c->landed, c->stream));
        const double T3 = now_s();
        CTO_HIP(wait_event(c->landed));
        const double T4 = now_s();
        if ((rc = all_inflated()) != CTO_OK) return rc;
        rc = cto_pack_from_bam_inflated(j.bam_path, nullptr, ctg.c_str(), lo, hi, iv.empty() ? nullptr : iv.data(), int64_t(iv.size() / 2), s->ref.data(),
                                        s->ref_start, s->ref.size(), 2316, 0, cfg->max_depth, cfg->max_indel_length,
                                        static_cast<const uint8_t*>(c->h_out.p), size_t(sp.out_bytes), blocks, n, &s->pack);
        if (timing)
            fprintf(stderr, "device inflate: %.1f MB in %lld blocks -> %.1f MB: read %.1f ms, scan + alloc %.1f, enqueue %.1f, on the device %.1f, pile-up %.1f\n",
                    nbytes / 1e6, (long long)n, sp.out_bytes / 1e6, (T1 - T0) * 1e3, (T2 - T1) * 1e3, (T3 - T2) * 1e3, (T4 - T3) * 1e3, (now_s() - T4) * 1e3);
        if (rc == CTO_OK) { *done = 1; ++device_inflated; }
        return rc;
    }

    // mpileup text (a mapped file, the slot's tokeniser buffer, samtools' output) -> the slot's pack: on the device where that is configured
    // and the text is one the single pass of cto_tokenise_device takes (*on_device: as adopt_device_pack leaves it), else on the host
    int pack_from_text(Slot* s, const char* text, size_t len, hipStream_t stream, bool* on_device) {
        *on_device = false;
        int rc;
        if (cfg->device_tokenise && len > 0) {
            cto_pack_view dvw{};
            cto_pack* lite = nullptr;
            int fallback = 0;
            if (!s->tok && (rc = cto_dev_tokeniser_create(&s->tok))) return rc;
            if ((rc = cto_tokenise_device(s->tok, text, len, s->ref.data(), s->ref_start, s->ref.size(), cfg->max_indel_length, stream, &dvw, &lite, &fallback)))
                return rc;
            if (!fallback) {
                // waiting for s->uploaded: the site list left the staging buffer; the tokeniser's arrays are free for the next chunk
                if ((rc = adopt_device_pack(s, dvw, lite, s->stage, stream, s->uploaded)) != CTO_OK) return rc;
                *on_device = true;
                ++device_tokenised;
                return CTO_OK;
            }
        }
        // the tokeniser's threads merge their entries straight into the staging buffer (a read-base is >= 3 characters of text)
        const size_t ecap = len / 3 + 4096;
        if ((rc = s->stage.ensure(ecap * 4 + len / 4 + (size_t(1) << 20))) != CTO_OK) return rc;
        return pack_from_mpileup_impl(len ? text : "", len, s->ref.data(), s->ref_start, s->ref.size(), cfg->max_indel_length,
                                      static_cast<uint32_t*>(s->stage.p), ecap, &s->pack);
    }

    // the pack of a chunk whose pileup is a text file; false: failed (the error is recorded)
    bool pack_from_text_file(Slot* s, const cto_chunk_job& j, hipStream_t stream, bool* on_device) {
        const size_t pl = strlen(j.mpileup_path);
        const bool gz = pl > 3 && strcmp(j.mpileup_path + pl - 3, ".gz") == 0;
        int rc;
        if (cfg->device_tokenise && !gz) {
            // the file is read straight into the tokeniser's page-locked buffer: no mapping, no staging copy
            if (!s->tok && cto_dev_tokeniser_create(&s->tok) != CTO_OK) { fail(cto_last_error()); return false; }
            const File f(j.mpileup_path);
            if (!f.ok()) { fail(std::string("cannot open ") + j.mpileup_path); return false; }
            size_t tn = 0;
            if (!f.size(&tn)) { fail(std::string("cannot stat ") + j.mpileup_path); return false; }
            char* buf = cto_dev_tokeniser_buffer(s->tok, tn + 1);
            if (!buf) { fail(cto_last_error()); return false; }
            if (!read_exact(f.fd, buf, tn, 0)) { fail(std::string("short read of ") + j.mpileup_path); return false; }
            rc = pack_from_text(s, buf, tn, stream, on_device);
        } else {
            Mapped txt;
            std::string err;
            if (!txt.open(j.mpileup_path, &err)) { fail(err); return false; }
            rc = pack_from_text(s, txt.p, txt.n, stream, on_device);
        }
        if (rc != CTO_OK) { fail(cto_last_error()); return false; }
        return true;
    }

    // the pack of a chunk piled up from the BAM (lo..hi, only `iv` when not empty) by a samtools child, the device or the host reader
    bool pack_from_alignments(Slot* s, const cto_chunk_job& j, const std::string& ctg, bool region_job, int64_t lo, int64_t hi, const std::vector<int64_t>& iv,
                              hipStream_t stream, bool* on_device) {
        int rc = CTO_OK;
        if (cfg->samtools) {
            // the reference's own producer: `samtools mpileup` with --min-BQ 0 (one pileup serves both passes), its text tokenised
            std::vector<std::string> cmd = {cfg->samtools, "mpileup", "--reverse-del", "--output-MQ", "-r",
                                            ctg + ":" + std::to_string(lo) + "-" + std::to_string(hi), "--min-MQ", "0", "--min-BQ", "0"};
            if (!region_job) { cmd.push_back("-l"); cmd.push_back(j.bed_path); }      // the reference's order of options
            cmd.push_back("--excl-flags");
            cmd.push_back("2316");
            if (cfg->samtools_max_depth > 0) { cmd.push_back("--max-depth"); cmd.push_back(std::to_string(cfg->samtools_max_depth)); }
            cmd.push_back(j.bam_path);
            std::vector<char> text;
            std::string err;
            if (!capture_stdout(cmd, &text, &err)) { fail(err); return false; }
            rc = pack_from_text(s, text.data(), text.size(), stream, on_device);
        } else {
            InflateCtx* c = nullptr;
            int done = 0;
            // a device-inflate context is free: this chunk's blocks go to the GPU.  A REGION job waits for one: piled up at every
            // position it is seven times a BED chunk's work, which the host reader needs most of a second of a core for
            // A BED chunk does not wait (CTO_CTX_WAIT_MS, default 0): measured with 96 chunks, waiting 0 / 10 / 20 / 40 ms for a context
            // sends 68 / 72 / 72 / 80 of them through the device and gives 667 / 654 / 646 / 612 k sites/s - for BED chunks the device
            // is the busier side, the cores take what it cannot
            static const int ctx_wait_ms = [] { const char* e = getenv("CTO_CTX_WAIT_MS"); return e ? atoi(e) : 0; }();
            if (free_ctx.pop(&c, inflate_ctx.empty() ? 0 : region_job && cfg->device_pileup ? -1 : std::max(ctx_wait_ms, 0))) {
                rc = pack_from_bam_device(j, ctg, lo, hi, iv, s, c, &done);
                free_ctx.push(c);
                *on_device = rc == CTO_OK && done == 2;
            }
            if (!done && rc == CTO_OK)
                rc = cto_pack_from_bam(j.bam_path, nullptr, ctg.c_str(), lo, hi, iv.empty() ? nullptr : iv.data(), int64_t(iv.size() / 2),
                                       s->ref.data(), s->ref_start, s->ref.size(), 2316, 0, cfg->max_depth, cfg->max_indel_length, &s->pack);
        }
        if (rc != CTO_OK) { fail(cto_last_error()); return false; }
        return true;
    }

    bool nothing_to_call(const cto_chunk_job& j) { if (cfg->verbose) fprintf(stderr, "[INFO] %s total processed positions: 0\n", j.ctg_name); return false; }

    // host half of a chunk + the upload; false = nothing to call in this chunk (no output) or an error (failed is set)
    bool produce(Slot* s, hipStream_t stream) {
        const cto_chunk_job& j = jobs[s->job];
        const std::string ctg = j.ctg_name;
        const bool region_job = j.bed_path == nullptr;           // candidates are extracted from the pile-up, not read from a BED
        std::string err;
        Mapped bed;
        int64_t ctg_start = 0, ctg_end = 0;
        int64_t cand_lo = 0, cand_hi = 0;                        // REGION job: rows of this range take part in the extraction
        if (region_job) {
            ctg_start = std::max<int64_t>(1, j.region_start);
            ctg_end = j.region_end;
            // extract_candidates_calling.py:289-292: reads (and therefore rows, and candidates) of ctg_start - 33 .. ctg_end + 33
            cand_lo = std::max<int64_t>(ctg_start - FLANK_POS, 1);
            cand_hi = ctg_end + FLANK_POS;
            s->sites.clear();
        } else {
            if (!bed.open(j.bed_path, &err)) { fail(err); return false; }
            std::vector<int32_t> centres(std::count(bed.p, bed.p + bed.n, '\n') + 2);
            int64_t span[2] = {0, 0};
            int has_types = 0;
            const int64_t n = cto_bed_centres(bed.p ? bed.p : "", bed.n, ctg.c_str(), centres.data(), int64_t(centres.size()), span, &has_types);
            if (n < 0) { fail(cto_last_error()); return false; }
            centres.resize(size_t(n));
            std::sort(centres.begin(), centres.end());
            centres.erase(std::unique(centres.begin(), centres.end()), centres.end());
            s->sites.swap(centres);
            candidates += int64_t(s->sites.size());
            if (s->sites.empty()) return nothing_to_call(j);
            ctg_start = span[0];
            ctg_end = span[1];
        }
        s->ref_start = std::max<int64_t>(1, ctg_start - EXPAND_REF);
        FaiRec fr;
        if (!fai_of(ctg, &fr, &err) || !read_region(fasta, fr, s->ref_start, ctg_end + EXPAND_REF, &s->ref, &err)) { fail(err); return false; }
        if (s->ref.empty()) { fail(std::string("[ERROR] Failed to load reference sequence from file (") + cfg->ref_fa + ")."); return false; }
        s->drop_pack();
        bool piled_on_device = false;
        const double t_pack = now_s();
        if (j.mpileup_path) {
            if (!pack_from_text_file(s, j, stream, &piled_on_device)) return false;
        } else {
            std::vector<int64_t> iv;                               // REGION job: every position of the range (no -l)
            if (!region_job) bed_intervals(bed.p ? bed.p : "", bed.n, ctg, &iv);
            // REGION job: the candidate range + the flanks of the windows at its edges
            const int64_t lo = region_job ? std::max<int64_t>(1, cand_lo - REGION_FLANK) : std::max<int64_t>(1, ctg_start - FLANK_POS);
            const int64_t hi = region_job ? cand_hi + REGION_FLANK : ctg_end + FLANK_POS;
            if (!pack_from_alignments(s, j, ctg, region_job, lo, hi, iv, stream, &piled_on_device)) return false;
        }
        if (piled_on_device) {               // the pack is in the slot's device buffers already (adopt_device_pack), s->uploaded recorded
            std::lock_guard<std::mutex> g(stat_m);
            st.pack_s += now_s() - t_pack;
        } else {
            if (cto_pack_view_of(s->pack, &s->hv) != CTO_OK) { fail(cto_last_error()); return false; }
            const double t_up = now_s();
            if (!upload(s, stream)) return false;
            std::lock_guard<std::mutex> g(stat_m);
            st.pack_s += t_up - t_pack;
            st.upload_s += now_s() - t_up;
        }
        return region_job ? extract_sites(s, j, cand_lo, cand_hi, stream) : true;
    }

    // One copy per chunk out of a page-locked staging buffer.  (hipMemcpyAsync from the pack's pageable arrays goes through the
    // runtime's own staging buffer, which every producer thread shares: measured, 8 producers spent 2.4 ms per chunk in those
    // calls, 16 producers 6.6 ms, and the whole pipeline levelled off at ~8.5 GB/s of uploads = 1.4-1.6 M sites/s.)
    bool upload(Slot* s, hipStream_t stream) {
        const cto_pack_view& h = s->hv;
        const PackLayout lay(h, s->sites.data(), s->sites.size());
        const bool in_place = h.entries == s->stage.p && h.n_entries > 0;          // entries first: already there for the text producer
        if (s->stage.grow_keeping(lay.total, in_place ? lay.bytes[0] : 0) != CTO_OK || s->pack_dev.ensure(lay.total) != CTO_OK) { fail(cto_last_error()); return false; }
        char* hs = static_cast<char*>(s->stage.p);
        if (in_place) {                      // grow_keeping may have moved the staging buffer: nothing may keep pointing at the old one
            s->pack->ext_entries = reinterpret_cast<uint32_t*>(hs);
            s->hv.entries = reinterpret_cast<const uint32_t*>(hs);
        }
        lay.stage(hs, in_place ? 1 : 0);
        if (hipMemcpyAsync(s->pack_dev.p, hs, lay.total, hipMemcpyHostToDevice, stream) != hipSuccess) { fail("hipMemcpyAsync failed"); return false; }
        s->dv = h;
        lay.bind(s->pack_dev.p, &s->dv, &s->d_site_pos);
        if (hipEventRecord(s->uploaded, stream) != hipSuccess) { fail("hipEventRecord failed"); return false; }
        return true;
    }

    // REGION job: STEP 1 of the reference on the pack that is now in HBM (the gates of extract_candidates_calling.py:55-169 as
    // cto_extract_candidates runs them, the candidate list of :433-446 compacted on the device in position order).  The positions
    // stay in HBM as the chunk's site list and come to the host once (the writers print them); false = no candidate (no output).
    bool extract_sites(Slot* s, const cto_chunk_job& j, int64_t cand_lo, int64_t cand_hi, hipStream_t stream) {
        const double t0 = now_s();
        const int64_t nc = s->hv.n_cols;
        if (nc == 0) {
            if (j.candidates_path) { FILE* f = fopen(j.candidates_path, "w"); if (f) fclose(f); }
            if (j.hybrid_info_path) { FILE* f = fopen(j.hybrid_info_path, "w"); if (f) fclose(f); }
            return nothing_to_call(j);
        }
        const int64_t nb = cdiv(nc, 256);
        if (s->xflags.ensure(size_t(nc)) != CTO_OK || s->xdepth.ensure(size_t(nc) * 4) != CTO_OK ||
            s->xscratch.ensure(size_t(std::max<int64_t>(s->hv.n_keys, 1)) * 4) != CTO_OK || s->cand.ensure(size_t(nc) * 4 + 256) != CTO_OK ||
            s->cand_scr.ensure(size_t(nb + 2) * 4) != CTO_OK || s->cand_host.ensure(size_t(nc) * 4 + 256) != CTO_OK) {
            fail(cto_last_error());
            return false;
        }
        const bool indel = cfg->K == 6;
        int32_t* d_n = static_cast<int32_t*>(s->cand_scr.p) + nb + 1;
        int rc = extract_candidates_scratch(&s->dv, cfg->extract_min_mq, cfg->extract_min_bq, cfg->snv_min_af, indel ? cfg->indel_min_af : 1.0,
                                            cfg->min_coverage, cfg->alt_base_num, indel ? 1 : 0, static_cast<uint32_t*>(s->xscratch.p),
                                            static_cast<uint8_t*>(s->xflags.p), static_cast<int32_t*>(s->xdepth.p), stream);
        // the other modes of extract_candidates_calling, each on the flags in HBM and in the reference's order: rows outside the confident
        // BED do not exist (`samtools mpileup -l`, :302); indel candidates only inside --call_indels_only_in_these_regions (:437-446; the
        // user's own --bed_fn supersedes it, :438); positions of the hybrid / genotyping VCF are marked (:347-349, 370-383)
        const std::vector<int64_t>* indel_iv = nullptr;
        if (indel && !cfg->indel_bed_superseded) {
            const auto it = indel_regions.find(j.ctg_name);
            if (it != indel_regions.end()) indel_iv = &it->second;
        }
        const int64_t n_conf = j.restrict_to_confident ? std::max<int64_t>(j.n_confident_intervals, 0) : 0;
        const int64_t n_indel_iv = indel_iv ? int64_t(indel_iv->size() / 2) : 0;
        int64_t k_lo = 0, k_hi = 0;                    // the known positions inside the rows that take part
        if (j.known_pos && j.n_known_pos > 0) {
            k_lo = std::lower_bound(j.known_pos, j.known_pos + j.n_known_pos, int32_t(std::min<int64_t>(cand_lo, INT32_MAX))) - j.known_pos;
            k_hi = std::upper_bound(j.known_pos, j.known_pos + j.n_known_pos, int32_t(std::min<int64_t>(cand_hi, INT32_MAX))) - j.known_pos;
        }
        const int64_t n_known = k_hi - k_lo;
        const bool want_info = j.hybrid_info_path != nullptr;
        const size_t nk_pack = size_t(std::max<int64_t>(s->hv.n_keys, 1));
        // layout of xmode (int32 words): confident pairs | indel pairs | known positions | records [n_known][16] | gcnt [n_keys] | gfirst [n_keys]
        const size_t w_conf = 0, w_indel = w_conf + size_t(2 * n_conf), w_known = w_indel + size_t(2 * n_indel_iv), w_rec = w_known + size_t(n_known),
                     w_gcnt = w_rec + (want_info ? size_t(n_known) * 16 : 0), w_gfirst = w_gcnt + (want_info && indel ? nk_pack : 0),
                     w_end = w_gfirst + (want_info && indel ? nk_pack : 0);
        int32_t* xm = nullptr;
        int32_t* xh = nullptr;
        if (rc == CTO_OK && (j.restrict_to_confident || n_indel_iv > 0 || n_known > 0)) {
            if (s->xmode.ensure(w_end * 4 + 256) != CTO_OK || s->xmode_host.ensure(w_end * 4 + 256) != CTO_OK) { fail(cto_last_error()); return false; }
            xm = static_cast<int32_t*>(s->xmode.p);
            xh = static_cast<int32_t*>(s->xmode_host.p);
            if (n_conf > 0) memcpy(xh + w_conf, j.confident_intervals, size_t(2 * n_conf) * 4);
            for (int64_t i = 0; i < 2 * n_indel_iv; ++i) xh[w_indel + size_t(i)] = int32_t(std::min<int64_t>((*indel_iv)[size_t(i)], INT32_MAX));
            if (n_known > 0) memcpy(xh + w_known, j.known_pos + k_lo, size_t(n_known) * 4);
            if (w_rec > 0 && hipMemcpyAsync(xm, xh, w_rec * 4, hipMemcpyHostToDevice, stream) != hipSuccess) { fail("hipMemcpyAsync failed"); return false; }
            if (j.restrict_to_confident)
                rc = cto_extract_restrict(&s->dv, static_cast<uint8_t*>(s->xflags.p), static_cast<int32_t*>(s->xdepth.p), xm + w_conf, int(n_conf), 0xff, stream);
            if (rc == CTO_OK && n_indel_iv > 0)
                rc = cto_extract_restrict(&s->dv, static_cast<uint8_t*>(s->xflags.p), nullptr, xm + w_indel, int(n_indel_iv), 2 | 16, stream);
            if (rc == CTO_OK && n_known > 0)
                rc = cto_extract_mark(&s->dv, static_cast<uint8_t*>(s->xflags.p), xm + w_known, int(n_known), 64, stream);
            if (rc == CTO_OK && want_info && n_known > 0) {
                if (indel && hipMemsetAsync(xm + w_gcnt, 0, 2 * nk_pack * 4, stream) != hipSuccess) { fail("hipMemsetAsync failed"); return false; }
                rc = cto_hybrid_info(&s->dv, static_cast<const uint8_t*>(s->xflags.p), xm + w_known, int(n_known), cfg->extract_min_mq, cfg->extract_min_bq,
                                     indel ? 1 : 0, xm + w_rec, indel ? reinterpret_cast<uint32_t*>(xm + w_gcnt) : nullptr, indel ? xm + w_gfirst : nullptr, stream);
                if (rc == CTO_OK && hipMemcpyAsync(xh + w_rec, xm + w_rec, (w_end - w_rec) * 4, hipMemcpyDeviceToHost, stream) != hipSuccess) {
                    fail("hipMemcpyAsync failed");
                    return false;
                }
            }
        }
        if (rc == CTO_OK)
            rc = cto_candidate_positions(&s->dv, static_cast<const uint8_t*>(s->xflags.p), indel ? 2 : 1, int32_t(std::min<int64_t>(cand_lo, INT32_MAX)),
                                         int32_t(std::min<int64_t>(cand_hi, INT32_MAX)), static_cast<int32_t*>(s->cand.p), nc,
                                         static_cast<int32_t*>(s->cand_scr.p), d_n, stream);
        if (rc != CTO_OK) { fail(cto_last_error()); return false; }
        auto* h = static_cast<int32_t*>(s->cand_host.p);
        if (hipMemcpyAsync(h, d_n, 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipEventRecord(s->uploaded, stream) != hipSuccess ||
            wait_event(s->uploaded) != hipSuccess) { fail("candidate extraction failed on the device"); return false; }
        int64_t n = h[0];
        candidates += n;
        if (n > 0) {
            if (hipMemcpyAsync(h, s->cand.p, size_t(n) * 4, hipMemcpyDeviceToHost, stream) != hipSuccess || hipEventRecord(s->uploaded, stream) != hipSuccess ||
                wait_event(s->uploaded) != hipSuccess) { fail("candidate extraction failed on the device"); return false; }
            s->sites.assign(h, h + n);
        }
        if (want_info) {                         // `<ctg>.<chunk>_hybrid_info` (:352-354, 490-497): counts from the device, strings here
            FILE* f = fopen(j.hybrid_info_path, "w");
            if (!f) { fail(std::string("cannot write ") + j.hybrid_info_path); return false; }
            if (n_known > 0) {
                const uint32_t* gc = indel ? reinterpret_cast<const uint32_t*>(xh + w_gcnt) : nullptr;
                const int32_t* gf = indel ? xh + w_gfirst : nullptr;
                const int64_t need = cto_hybrid_info_rows(s->pack, j.ctg_name, n_known, xh + w_known, xh + w_rec, indel ? 1 : 0, gc, gf, nullptr, 0);
                if (need < 0) { fclose(f); fail(cto_last_error()); return false; }
                std::vector<char> text(size_t(need) + 1);
                if (need > 0 && cto_hybrid_info_rows(s->pack, j.ctg_name, n_known, xh + w_known, xh + w_rec, indel ? 1 : 0, gc, gf, text.data(), size_t(need)) != need) {
                    fclose(f); fail(cto_last_error()); return false;
                }
                if (need > 0) fwrite(text.data(), 1, size_t(need), f);
            }
            if (fclose(f) != 0) { fail(std::string("short write to ") + j.hybrid_info_path); return false; }
        }
        s->d_site_pos = static_cast<const int32_t*>(s->cand.p);
        if (j.candidates_path) {                 // the reference's BED chunk rows (extract_candidates_calling.py:450-488), one file per region
            FILE* f = fopen(j.candidates_path, "w");
            if (!f) { fail(std::string("cannot write ") + j.candidates_path); return false; }
            for (int64_t i = 0; i < n; ++i) fprintf(f, "%s\t%d\t%d\n", j.ctg_name, std::max(h[i] - 17, 1), h[i] + 17);
            if (fclose(f) != 0) { fail(std::string("short write to ") + j.candidates_path); return false; }
        }
        { std::lock_guard<std::mutex> g(stat_m); st.pack_s += now_s() - t0; }
        return n > 0 || nothing_to_call(j);
    }

    // Tensor creation of one chunk on `main`: the [33][34] inputs of both networks (rows of x_aff / x_neg) and what the writers need of
    // the candidate columns (into the chunk's result buffer).
    // One kernel (a workgroup per candidate, the column histograms never leave LDS); CTO_FUSED_FEATURIZE=0 selects the two-stage path
    // through the per-column vectors in HBM (kept for A/B runs - same results).
    bool fused_featurize = true;
    int tensors(Slot* s, int64_t n, float* x_aff, float* x_neg, hipStream_t main) {
        int rc;
        void* rd = s->res_dev.p;
        int32_t* site_info = s->res.site_info(rd);
        // heavily overlapping windows (candidates a few bases apart) share most of their columns: the one-kernel path would histogram
        // them once per candidate, the two-stage path once (measured equal at ~8 columns per candidate; same results either way)
        if (fused_featurize && s->hv.n_cols >= 8 * n)
            return cto_featurize_sites(&s->dv, s->d_site_pos, n, cfg->min_bq, cfg->min_rescale_cov, x_aff, x_neg, nullptr, nullptr, site_info, s->res.colvec(rd),
                                       s->res.sitefirst(rd), s->res.keycnt(rd), s->res.keyfirst(rd), main);
        const size_t nc = size_t(std::max<int64_t>(s->hv.n_cols, 1));
        if ((rc = s->colvec.ensure(nc * CTO_COLVEC_STRIDE * 2)) || (rc = s->coldepth.ensure(nc * 8))) return rc;
        auto* colvec = static_cast<int16_t*>(s->colvec.p);
        if ((rc = cto_featurize_columns(&s->dv, cfg->min_bq, colvec, static_cast<int32_t*>(s->coldepth.p), s->res.keycnt(rd), main))) return rc;
        if ((rc = cto_gather_windows(&s->dv, colvec, static_cast<int32_t*>(s->coldepth.p), s->d_site_pos, n, cfg->min_bq, cfg->min_rescale_cov, x_aff,
                                     x_neg, nullptr, nullptr, site_info, s->res.sitefirst(rd), s->res.keyfirst(rd), main)))
            return rc;
        hipLaunchKernelGGL(k_gather_rows, dim3(unsigned(n)), dim3(128), 0, main, colvec, site_info, n, s->res.colvec(rd));
        CTO_HIP(hipGetLastError());
        return CTO_OK;
    }

    static constexpr size_t X_ROW = size_t(CTO_NPOS) * CTO_NCHAN;      // floats of one site's network input

    // What both launch modes begin a chunk with: its result layout and buffers, the wait for its upload, `begin`, tensor creation on `main`.
    // `carried` rows of earlier chunks (tile stream only) move to the front of the chunk's input buffers first, its own rows follow them.
    int begin_chunk(Slot* s, int64_t carried, hipStream_t main) {
        const int64_t n = int64_t(s->sites.size());
        const size_t row = X_ROW * 4;
        int rc;
        // everything the writers need goes into ONE device buffer and comes back with ONE copy on the copy-back stream: seven copies
        // queued behind the kernels on the launch stream cost ~0.1 ms per chunk in which the next chunk's kernels could not start
        s->res = ResultLayout(n, s->hv.n_keys);
        if ((rc = s->x_aff.ensure(size_t(carried + n) * row)) || (rc = s->x_neg.ensure(size_t(carried + n) * row)) ||
            (rc = s->res_dev.ensure(s->res.total)) || (rc = s->res_host.ensure(s->res.total)))
            return rc;
        CTO_HIP(hipStreamWaitEvent(main, s->uploaded, 0));
        CTO_HIP(hipEventRecord(s->begin, main));
        if (carried > 0) {
            CTO_HIP(hipMemcpyAsync(s->x_aff.p, static_cast<char*>(carry_home->x_aff.p) + size_t(carry_at) * row, size_t(carried) * row, hipMemcpyDeviceToDevice, main));
            if (!cfg->neg_reads_aff)
                CTO_HIP(hipMemcpyAsync(s->x_neg.p, static_cast<char*>(carry_home->x_neg.p) + size_t(carry_at) * row, size_t(carried) * row, hipMemcpyDeviceToDevice, main));
        }
        return tensors(s, n, static_cast<float*>(s->x_aff.p) + size_t(carried) * X_ROW, static_cast<float*>(s->x_neg.p) + size_t(carried) * X_ROW, main);
    }

    // room for the logits and posteriors of `m` rows (growing frees, and a free waits for the device: before a chunk queues anything)
    int grow_outputs(Slot* home, int64_t m) {
        const size_t b = size_t(cfg->K) * size_t(m) * 8;
        int rc;
        return (rc = home->la.ensure(b)) || (rc = home->ln.ensure(b)) ? rc : home->post.ensure(b);
    }

    // both networks and the epilogue over `m` rows of inputs on `main`; logits and posteriors stay in `home`'s buffers
    int networks(Slot* home, const float* x_aff, const float* x_neg, int64_t m, int32_t* decision, double* qual, hipStream_t main, cto_model* aff,
                 cto_model* neg) {
        const int K = cfg->K;
        int rc;
        if ((rc = cto_model_forward(neg, cfg->neg_reads_aff ? x_aff : x_neg, m, static_cast<float*>(home->ln.p), main))) return rc;
        if ((rc = cto_model_forward(aff, x_aff, m, static_cast<float*>(home->la.p), main))) return rc;
        return cto_posterior(static_cast<const float*>(home->la.p), static_cast<const float*>(home->ln.p), K, m, cfg->d_lik, cfg->d_edges, nullptr,
                             static_cast<double*>(home->post.p), decision, qual, main);
    }

    // the chunk's results, complete on `main`, go to the host on the copy-back stream; s->done follows them
    int send_back(Slot* s, hipStream_t main, hipStream_t copy_back) {
        CTO_HIP(hipEventRecord(s->computed, main));
        CTO_HIP(hipStreamWaitEvent(copy_back, s->computed, 0));
        CTO_HIP(hipMemcpyAsync(s->res_host.p, s->res_dev.p, s->res.total, hipMemcpyDeviceToHost, copy_back));
        CTO_HIP(hipEventRecord(s->done, copy_back));
        return CTO_OK;
    }

    // a chunk as a launch of its own: decision and QUAL are written straight into its result buffer
    int launch(Slot* s, hipStream_t main, hipStream_t copy_back, cto_model* aff, cto_model* neg) {
        const int64_t n = int64_t(s->sites.size());
        int rc;
        if ((rc = grow_outputs(s, n)) || (rc = begin_chunk(s, 0, main))) return rc;
        void* rd = s->res_dev.p;
        if ((rc = networks(s, static_cast<const float*>(s->x_aff.p), static_cast<const float*>(s->x_neg.p), n, s->res.decision(rd), s->res.qual(rd), main, aff, neg)))
            return rc;
        CTO_HIP(hipEventRecord(s->kernels_end, main));
        return send_back(s, main, copy_back);
    }

    // ---- the networks fed by a STREAM of sites instead of by chunks --------------------------------------------------------------
    // The recurrent kernels put 32 sites x one direction on a CU, so a launch is efficient when it is a whole number of rounds
    // (16 x CUs sites: 4096 on MI355X) and the reference's 10 000-site chunk files (shared/param.py:21) are 2.44 rounds of work in 2.83
    // rounds of time.  Sites are independent, so the launcher runs the networks on whole rounds only and carries the tail of a chunk
    // into the launch of the next one: the tail's input rows are copied to the front of the next chunk's input buffers, the
    // featurisation of that chunk appends behind them, and what the networks + the epilogue return is dealt back to the chunks it
    // belongs to (`pending`: chunk, first row, rows, in buffer order).  A chunk goes to the writers when its last row is back; what is
    // left at the end of the run (or when `max_pending` chunks are waiting - they hold slots the producers need) is launched as it is.
    struct Pending { Slot* s; int64_t row0, cnt; };
    std::vector<Pending> pending;
    Slot* carry_home = nullptr;              // whose x buffers hold the pending rows ...
    int64_t carry_at = 0;                    // ... starting at this row
    int64_t round_sites = 4096;
    size_t max_pending = 2;
    Event flush_begin, flush_end;            // created for a tile stream only
    bool flush_timed = false;

    int64_t pending_rows() const { int64_t c = 0; for (const Pending& q : pending) c += q.cnt; return c; }

    // networks + epilogue over rows [at, at + m) of `home`'s input buffers; results dealt out to the first m pending rows
    int run_networks(Slot* home, int64_t at, int64_t m, hipStream_t main, hipStream_t copy_back, cto_model* aff, cto_model* neg,
                     std::vector<Slot*>* complete, hipEvent_t kernels_end) {
        constexpr size_t DEC = ResultLayout::DECISION_ROW, QUAL = ResultLayout::QUAL_ROW;
        int rc;
        if ((rc = grow_outputs(home, m)) || (rc = home->dec_l.ensure(size_t(m) * DEC)) || (rc = home->qual_l.ensure(size_t(m) * QUAL))) return rc;
        if ((rc = networks(home, static_cast<const float*>(home->x_aff.p) + size_t(at) * X_ROW, static_cast<const float*>(home->x_neg.p) + size_t(at) * X_ROW, m,
                           static_cast<int32_t*>(home->dec_l.p), static_cast<double*>(home->qual_l.p), main, aff, neg)))
            return rc;
        if (kernels_end) CTO_HIP(hipEventRecord(kernels_end, main));   // before any chunk of this launch can reach a writer, which reads it
        int64_t o = 0;
        size_t used = 0;
        // chunks handed to *complete leave `pending` on EVERY way out of the loop (a failing HIP call returns from its middle): a
        // slot in both lists would be given back to the free list twice by the launcher's hand_over() + abandon_pending()
        struct ErasePrefix {
            std::vector<Pending>& v; size_t& n;
            ~ErasePrefix() { v.erase(v.begin(), v.begin() + long(n)); }
        } erase_prefix{pending, used};
        for (Pending& q : pending) {
            if (o >= m) break;
            const int64_t take = std::min(q.cnt, m - o);
            void* rd = q.s->res_dev.p;
            CTO_HIP(hipMemcpyAsync(reinterpret_cast<char*>(q.s->res.decision(rd)) + size_t(q.row0) * DEC, static_cast<char*>(home->dec_l.p) + size_t(o) * DEC,
                                   size_t(take) * DEC, hipMemcpyDeviceToDevice, main));
            CTO_HIP(hipMemcpyAsync(reinterpret_cast<char*>(q.s->res.qual(rd)) + size_t(q.row0) * QUAL, static_cast<char*>(home->qual_l.p) + size_t(o) * QUAL,
                                   size_t(take) * QUAL, hipMemcpyDeviceToDevice, main));
            q.row0 += take;
            q.cnt -= take;
            o += take;
            if (q.cnt == 0) {
                if ((rc = send_back(q.s, main, copy_back))) return rc;
                complete->push_back(q.s);
                ++used;
            }
        }
        return CTO_OK;
    }

    // one chunk into the stream; chunks whose last row came back go to *complete (in chunk order)
    int launch_stream(Slot* s, hipStream_t main, hipStream_t copy_back, cto_model* aff, cto_model* neg, std::vector<Slot*>* complete) {
        const int64_t n = int64_t(s->sites.size()), c = pending_rows();
        int rc;
        if ((rc = begin_chunk(s, c, main))) return rc;       // the rows still waiting move to the front of this chunk's input buffers
        pending.push_back({s, 0, n});
        carry_home = s;
        carry_at = 0;
        const int64_t all = c + n;
        const int64_t m = pending.size() > max_pending ? all : all / round_sites * round_sites;
        if (m > 0) {
            if ((rc = run_networks(s, 0, m, main, copy_back, aff, neg, complete, s->kernels_end))) return rc;
            carry_at = m;
        } else {
            CTO_HIP(hipEventRecord(s->kernels_end, main));
        }
        return CTO_OK;
    }

    // the end of the run: what is still waiting is launched as it is
    int flush_stream(hipStream_t main, hipStream_t copy_back, cto_model* aff, cto_model* neg, std::vector<Slot*>* complete) {
        const int64_t c = pending_rows();
        if (c == 0) { for (const Pending& q : pending) complete->push_back(q.s); pending.clear(); return CTO_OK; }
        if (flush_begin.e) CTO_HIP(hipEventRecord(flush_begin, main));
        const int rc = run_networks(carry_home, carry_at, c, main, copy_back, aff, neg, complete, flush_end);
        if (rc == CTO_OK && flush_end.e) flush_timed = true;
        return rc;
    }

    // alt_info strings, VCF records, file
    bool finish(Slot* s) {
        const cto_chunk_job& j = jobs[s->job];
        if (wait_event(s->done) != hipSuccess) { fail("waiting for the chunk's results failed"); return false; }
        {
            float ms = 0;
            // the kernels this chunk's launch queued (with a tile stream, its own tail runs - and is counted - in the next chunk's launch)
            if (hipEventElapsedTime(&ms, s->begin, s->kernels_end) == hipSuccess) { std::lock_guard<std::mutex> g(stat_m); st.device_s += ms * 1e-3; }
        }
        const int64_t n = int64_t(s->sites.size());
        void* rh = s->res_host.p;
        int32_t* info = s->res.site_info(rh);
        const int32_t* h_decision = s->res.decision(rh);
        static const uint32_t zero_k[1] = {0};
        static const int32_t zero_kf[2] = {0, 0};
        const uint32_t* keycnt = s->hv.n_keys ? s->res.keycnt(rh) : zero_k;
        const int32_t* keyfirst = s->hv.n_keys ? s->res.keyfirst(rh) : zero_kf;
        std::vector<int64_t> alt_off(size_t(n) + 1, 0);
        std::vector<char> alt(size_t(256 * n + (1 << 16)));
        int64_t used = -1;
        for (int tries = 0; tries < 8; ++tries) {
            used = cto_alt_info_batch_sites(s->pack, n, info, 0, s->res.colvec(rh), s->res.sitefirst(rh),
                                            keycnt, keyfirst, alt.data(), alt.size(), alt_off.data());
            if (used >= 0) break;
            if (!strstr(cto_last_error(), "buffer too small")) break;
            alt.resize(alt.size() * 4);
        }
        if (used < 0) { fail(cto_last_error()); return false; }
        std::vector<char> centre(static_cast<size_t>(n));
        for (int64_t i = 0; i < n; ++i) {
            const int64_t at = int64_t(s->sites[size_t(i)]) - s->ref_start;
            const char c = at >= 0 && at < int64_t(s->ref.size()) ? s->ref[size_t(at)] : 'N';
            centre[size_t(i)] = c;
            if (c != 'A' && c != 'C' && c != 'G' && c != 'T') info[i * 12 + 3] |= 1;      // predict.py:219-228: centre not in ACGT -> no row
        }
        std::vector<char> text(size_t(512 * std::max<int64_t>(n, 1) + 2 * used + 4096));
        int64_t counts[4] = {0, 0, 0, 0};
        int64_t tu = -1;
        for (int tries = 0; tries < 6; ++tries) {
            tu = cto_vcf_rows_batch(j.ctg_name, n, s->sites.data(), centre.data(), alt.data(), alt_off.data(), info, h_decision,
                                    s->res.qual(rh), cfg->K, cfg->show_ref, cfg->qual_pass, text.data(), text.size(), counts);
            if (tu != CTO_ENOMEM) break;
            text.resize(text.size() * 4);
        }
        if (tu < 0) { fail(cto_last_error()); return false; }
        if (counts[0] > 0) {              // the reference removes VCFs without records (call_variants.py:859-867)
            FILE* f = fopen(j.vcf_path, "w");
            if (!f) { fail(std::string("cannot write ") + j.vcf_path); return false; }
            const size_t hl = strlen(cfg->vcf_header);
            const bool ok = fwrite(cfg->vcf_header, 1, hl, f) == hl && fwrite(text.data(), 1, size_t(tu), f) == size_t(tu);
            if (fclose(f) != 0 || !ok) { fail(std::string("short write to ") + j.vcf_path); return false; }
        } else {
            (void)unlink(j.vcf_path);
        }
        if (cfg->verbose) {
            for (int64_t i = 0; i < counts[2]; ++i) puts("low tumor coverage");             // call_variants.py:328, one line per such site
            if (counts[3]) {
                const int32_t* dec = h_decision;
                for (int64_t i = 0; i < n; ++i)
                    if (dec[i * 4 + 1] & 3)
                        fprintf(stderr, "[WARNING] %s:%d a probability printed as 1.00000000 / 0.00000000 falls outside the likelihood bins (the "
                                "reference raises IndexError here); %s\n", j.ctg_name, s->sites[size_t(i)],
                                (dec[i * 4 + 1] & 2) ? "no posterior, site skipped" : "bin clamped");
            }
            fprintf(stderr, "[INFO] %s total processed positions: %lld\n", j.ctg_name, (long long)counts[1]);
        }
        rows += counts[0];
        sites += counts[1];
        low_cov += counts[2];
        clamped += counts[3];
        return true;
    }

    // ---- the three kinds of thread -------------------------------------------------------------------------------------------------
    // a producer: chunks from the job list into free slots, on `shared` (a copy stream of several producers) or a stream of its own
    void producer(int dev, hipStream_t shared) {
        Stream own;
        hipStream_t copy = shared;
        tl_pack_threads = cfg->pack_threads;                     // the tokeniser's / BAM decoder's own threads per call
        if (shared) (void)hipSetDevice(dev);
        else if (hipSetDevice(dev) != hipSuccess || own.create() != CTO_OK) fail("producer: no HIP stream");
        else copy = own;
        for (;;) {
            if (failed) break;
            const int64_t j = next_job.fetch_add(1);
            if (j >= n_jobs) break;
            Slot* s = nullptr;
            if (!free_slots.pop(&s)) break;
            if (failed) {                                        // the run failed while this thread waited for a slot: what the slot's
                free_slots.push(s);                              // last chunk queued on the device may still be running - leave it alone
                break;
            }
            s->job = j;
            const double t0 = now_s();
            bool ok = false;
            try {
                ok = copy && produce(s, copy);
            } catch (const std::exception& e) {                  // bad_alloc on a huge chunk: an error of the run, not of the process
                fail(std::string("producer: ") + e.what());
            }
            { std::lock_guard<std::mutex> g(stat_m); st.produce_s += now_s() - t0; }
            if (ok) to_launch.push(s);
            else free_slots.push(s);                             // nothing to call here (or an error: `failed` is set)
        }
        if (copy) (void)hipStreamSynchronize(copy);
    }

    void writer(int dev) {
        (void)hipSetDevice(dev);
        Slot* s = nullptr;
        while (to_write.pop(&s)) {
            const double t0 = now_s();
            try {
                if (!failed) finish(s);
            } catch (const std::exception& e) {
                fail(std::string("writer: ") + e.what());
            }
            { std::lock_guard<std::mutex> g(stat_m); st.finish_s += now_s() - t0; }
            free_slots.push(s);
        }
    }

    // the launcher (the calling thread): every chunk the producers deliver goes to the device - as a launch of its own, on `main` and
    // `second` in turn, or into the tile stream on `main` - and from there to the writers; returns when the producers are done
    int launcher(hipStream_t main, hipStream_t second, hipStream_t copy_back, bool tile_stream) {
        int rc = CTO_OK;
        int64_t launched = 0;
        std::vector<Slot*> complete;
        auto hand_over = [&] { for (Slot* c : complete) (failed ? free_slots : to_write).push(c); complete.clear(); };
        auto abandon_pending = [&] {             // a failed run: the chunks still waiting for rows give their slots back
            if (!pending.empty()) (void)hipStreamSynchronize(main);
            for (const Pending& q : pending) free_slots.push(q.s);
            pending.clear();
        };
        for (;;) {
            Slot* s = nullptr;
            const double t0 = now_s();
            if (!to_launch.pop(&s)) break;
            const double t1 = now_s();
            st.launcher_wait_s += t1 - t0;
            bool queued = false;
            if (!failed) {
                int r;
                if (tile_stream) {
                    r = launch_stream(s, main, copy_back, cfg->aff, cfg->neg, &complete);
                    queued = r == CTO_OK || std::any_of(pending.begin(), pending.end(), [s](const Pending& q) { return q.s == s; });
                } else {
                    const bool odd = second && (launched++ & 1);
                    r = launch(s, odd ? second : main, copy_back, odd ? cfg->aff2 : cfg->aff, odd ? cfg->neg2 : cfg->neg);
                    if (r == CTO_OK) { complete.push_back(s); queued = true; }
                }
                if (r != CTO_OK) { fail(cto_last_error()); rc = r; }
            }
            st.launch_s += now_s() - t1;
            if (!queued) {
                (void)hipStreamSynchronize(main);                         // its buffers may be in use by what was queued before the failure
                free_slots.push(s);
            }
            hand_over();
            if (failed) abandon_pending();
        }
        if (tile_stream && !failed) {
            const double t1 = now_s();
            const int r = flush_stream(main, copy_back, cfg->aff, cfg->neg, &complete);
            if (r != CTO_OK) { fail(cto_last_error()); rc = r; }
            st.launch_s += now_s() - t1;
            hand_over();
        }
        if (failed) abandon_pending();
        return rc;
    }
};

int check_arguments(const cto_run_cfg* cfg, const cto_chunk_job* jobs, int64_t n_jobs) {
    CTO_REQUIRE(cfg && (jobs || n_jobs == 0) && cfg->aff && cfg->neg && cfg->d_lik && cfg->d_edges && cfg->ref_fa && cfg->vcf_header, CTO_EINVAL,
                "cto_run_chunks: null argument");
    CTO_REQUIRE(cfg->K == 4 || cfg->K == 6, CTO_EINVAL, "cto_run_chunks: K must be 4 or 6");
    for (int64_t i = 0; i < n_jobs; ++i)
        CTO_REQUIRE(jobs[i].ctg_name && jobs[i].vcf_path && (jobs[i].mpileup_path || jobs[i].bam_path) &&
                        (jobs[i].bed_path || (jobs[i].region_start >= 0 && jobs[i].region_end >= std::max<int64_t>(jobs[i].region_start, 1))),   // a first chunk of --chunk_id starts at 0 (:262)
                    CTO_EINVAL, "cto_run_chunks: job %lld is incomplete", (long long)i);
    return CTO_OK;
}

// `depth` slots of device `dev` for the run: from the cache, the rest new
int lease_slots(Run& run, Lease<Slot>& lease, int dev, int depth) {
    lease.take(depth, [dev](const Slot& s) { return s.device == dev; });
    while (int(run.slots.size()) < depth) {
        run.slots.emplace_back(new Slot());
        if (const int rc = run.slots.back()->open(dev)) return rc;
    }
    for (auto& sl : run.slots) run.free_slots.push(sl.get());
    return CTO_OK;
}

// device-inflate contexts (BAM jobs only), kept across calls like the slots
void lease_inflate_contexts(Run& run, Lease<InflateCtx>& lease, int dev) {
    const cto_run_cfg* cfg = run.cfg;
    bool any_bam = false;
    for (int64_t i = 0; i < run.n_jobs; ++i) any_bam = any_bam || !run.jobs[i].mpileup_path;
    if (!any_bam || cfg->inflate_cus <= 0 || cfg->inflate_jobs <= 0) return;
    int n_cu = 256;
    (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
    const int cus = std::max(8, std::min(cfg->inflate_cus, n_cu * 3 / 4));      // the networks keep at least a quarter of the chip
    lease.take(cfg->inflate_jobs, [dev, cus](const InflateCtx& c) { return c.device == dev && c.cus == cus; });
    while (int(run.inflate_ctx.size()) < cfg->inflate_jobs) {
        run.inflate_ctx.emplace_back(new InflateCtx());
        if (run.inflate_ctx.back()->open(dev, cus) != CTO_OK) {           // no CU-masked streams on this runtime: host inflate only
            if (cfg->verbose) fprintf(stderr, "[WARNING] device inflate disabled: %s\n", cto_last_error());
            run.inflate_ctx.clear();
            break;
        }
    }
    for (auto& c : run.inflate_ctx) run.free_ctx.push(c.get());
}

// The streams of one call, declared before the threads that queue on them: they go (Stream drains, then destroys) after those are
// joined, on every way out of run_chunks()
struct RunStreams {
    Stream own_main, copy_back, second;
    std::vector<Stream> copy;                // the producers' shared copy streams
    hipStream_t main = nullptr;
    // `stream` waits for what is queued on `on` so far
    static int order_behind(hipStream_t stream, hipStream_t on) {
        Event before;
        if (const int rc = before.create(hipEventDisableTiming)) return rc;
        CTO_HIP(hipEventRecord(before, on));
        CTO_HIP(hipStreamWaitEvent(stream, before, 0));
        return CTO_OK;
    }
    int open(const cto_run_cfg* cfg, hipStream_t callers) {
        int rc;
        main = callers;
        if (!main) {
            // The legacy default stream synchronises with every blocking stream - the CU-masked inflate streams are such - and the networks
            // and the inflate launches would exclude each other in time (measured: BAM -> VCF 350 k instead of 400-490 k sites/s).  The
            // kernels get a non-blocking stream of this call, ordered behind what the caller has queued on the default stream so far.
            if ((rc = own_main.create()) || (rc = order_behind(own_main, nullptr))) return rc;
            main = own_main;
        }
        if ((rc = copy_back.create())) return rc;
        // a second compute stream for every other chunk, when the caller brought a second pair of handles (cto_run_cfg.aff2)
        if (cfg->aff2 && cfg->neg2 && ((rc = second.create()) || (rc = order_behind(second, main)))) return rc;
        return CTO_OK;
    }

    // The producers share TWO copy streams (CTO_COPY_STREAMS=n; 0: a stream each, as until the end of round 6).  The runtime maps a process's
    // streams onto four hardware queues; with a stream per producer the stream the networks run on shares its queue with one or two copy
    // streams, whose waits (a copy's completion) then stand in front of the networks' launches.  Two interleaved A/B runs of every file-to-file
    // leg: text -> VCF 1.97-1.98 -> 2.04-2.06 M sites/s, with the device tokeniser 1.85 -> 1.93-1.96 M, all-device BAM on two cores 0.56-0.58
    // -> 0.59-0.60 M, BAM -> VCF, REGION jobs and 10 000-site chunks unchanged.  A producer only queues on its stream and waits on its own
    // events, so what another producer queues in between costs it little.
    int open_copy_streams() {
        static const int shared_n = [] { const char* e = getenv("CTO_COPY_STREAMS"); return e ? atoi(e) : 2; }();
        std::vector<Stream> v(size_t(std::max(shared_n, 0)));
        copy.swap(v);
        for (Stream& c : copy)
            if (const int rc = c.create()) return rc;
        return CTO_OK;
    }
};

}  // namespace

static int run_chunks(const cto_run_cfg* cfg, const cto_chunk_job* jobs, int64_t n_jobs, void* stream, cto_run_stats* stats) {
    int rc;
    if ((rc = check_arguments(cfg, jobs, n_jobs)) != CTO_OK) return rc;
    if (stats) memset(stats, 0, sizeof(*stats));
    if (n_jobs == 0) return CTO_OK;
    const int producers = std::max(1, cfg->producers), writers = std::max(1, cfg->writers);
    const int depth = cfg->depth > 0 ? cfg->depth : producers + writers + 2;
    Run run{cfg, jobs, n_jobs};
    std::string err;
    CTO_REQUIRE(run.fasta.open(cfg->ref_fa, &err), CTO_EINVAL, "cto_run_chunks: %s", err.c_str());
    CTO_REQUIRE(!cfg->indel_regions_bed || !cfg->indel_regions_bed[0] || load_indel_regions(cfg->indel_regions_bed, &run.indel_regions, &err), CTO_EINVAL,
                "cto_run_chunks: %s", err.c_str());
    int dev = 0;
    CTO_HIP(hipGetDevice(&dev));
    Lease<Slot> slots_back{slot_cache(), &run.slots, [](Slot& s) { s.drop_pack(); }};
    if ((rc = lease_slots(run, slots_back, dev, depth)) != CTO_OK) return rc;
    Lease<InflateCtx> ctx_back{inflate_cache(), &run.inflate_ctx, nullptr};
    lease_inflate_contexts(run, ctx_back, dev);
    RunStreams streams;                      // (declared before the threads: destroyed after they are joined)
    if ((rc = streams.open(cfg, static_cast<hipStream_t>(stream))) != CTO_OK) return rc;
    const hipStream_t main = streams.main, second = streams.second, copy_back = streams.copy_back;
    const double t_begin = now_s();
    if ((rc = streams.open_copy_streams()) != CTO_OK) return rc;
    std::atomic<int> producers_left{producers};
    std::vector<std::thread> threads;
    threads.reserve(size_t(producers + writers));
    struct JoinAll {                         // whatever happens below, a started thread is joined (queues closed first: they all wake up)
        Run& run;
        std::vector<std::thread>& th;
        void join() {
            run.to_launch.close();
            run.to_write.close();
            run.free_slots.close();
            for (auto& t : th) if (t.joinable()) t.join();
        }
        ~JoinAll() { join(); }
    } join_all{run, threads};
    auto start = [&](auto&& body) -> bool {
        try {
            threads.emplace_back(std::forward<decltype(body)>(body));
            return true;
        } catch (const std::exception& e) {      // the system is out of threads
            run.fail(std::string("cannot start a thread: ") + e.what());
            return false;
        }
    };
    for (int t = 0; t < producers; ++t)
        if (!start([&run, &producers_left, dev, copy = streams.copy.empty() ? nullptr : streams.copy[size_t(t) % streams.copy.size()].s] {
            run.producer(dev, copy);
            if (--producers_left == 0) run.to_launch.close();
        })) {
            if (--producers_left == 0) run.to_launch.close();        // this one never ran
        }
    for (int t = 0; t < writers; ++t) (void)start([&run, dev] { run.writer(dev); });
    if (run.failed) run.free_slots.close();  // a thread did not start: nobody may wait for a slot that no writer will hand back
    // the networks take a stream of sites, not chunks (Run::launch_stream), unless two compute streams take the chunks in turn or the
    // caller turns it off (CTO_TILE_STREAM=0: every chunk is its own launch, as before)
    static const bool stream_off = [] { const char* e = getenv("CTO_TILE_STREAM"); return e && e[0] == '0'; }();
    const bool tile_stream = !second && !stream_off;
    static const bool fused_off = [] { const char* e = getenv("CTO_FUSED_FEATURIZE"); return e && e[0] == '0'; }();
    run.fused_featurize = !fused_off;
    if (tile_stream) {
        int n_cu = 256;
        (void)hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev);
        run.round_sites = int64_t(16) * std::max(n_cu, 1);
        // chunks that may wait for rows.  Each holds a slot, and a chunk only stops waiting when a LATER chunk is launched: with every
        // slot waiting no producer could ever deliver that chunk, so at most depth - 1 wait (the launch that would make it `depth`
        // takes everything that is pending instead)
        run.max_pending = size_t(std::max(0, std::min(4, depth - 1)));
        (void)run.flush_begin.create();      // without them the flush goes untimed
        (void)run.flush_end.create();
    }
    rc = run.launcher(main, second, copy_back, tile_stream);
    join_all.join();
    (void)hipStreamSynchronize(main);
    if (second) (void)hipStreamSynchronize(second);
    (void)hipStreamSynchronize(copy_back);
    if (run.flush_timed) {
        float ms = 0;
        if (hipEventElapsedTime(&ms, run.flush_begin, run.flush_end) == hipSuccess) run.st.device_s += ms * 1e-3;
    }
    if (stats) {
        *stats = run.st;
        stats->seconds = now_s() - t_begin;
        stats->candidates = run.candidates;
        stats->sites = run.sites;
        stats->rows = run.rows;
        stats->low_coverage = run.low_cov;
        stats->clamped = run.clamped;
        stats->device_inflated = run.device_inflated;
        stats->device_piled = run.device_piled;
        stats->device_tokenised = run.device_tokenised;
    }
    if (run.failed) {
        set_error("cto_run_chunks: %s", run.first_error.c_str());
        return rc != CTO_OK ? rc : CTO_EINVAL;
    }
    return CTO_OK;
}

// no C++ exception crosses the C ABI: what the set-up or the launcher thread throws (allocation failure) becomes an error code; the
// worker threads catch their own
extern "C" int cto_run_chunks(const cto_run_cfg* cfg, const cto_chunk_job* jobs, int64_t n_jobs, void* stream, cto_run_stats* stats) {
    try {
        return run_chunks(cfg, jobs, n_jobs, stream, stats);
    } catch (const std::bad_alloc&) {
        set_error("cto_run_chunks: out of memory");
        return CTO_ENOMEM;
    } catch (const std::exception& e) {
        set_error("cto_run_chunks: %s", e.what());
        return CTO_EINVAL;
    }
}

extern "C" int cto_run_release(void) {
    std::vector<std::unique_ptr<Slot>> drop;
    std::vector<std::unique_ptr<InflateCtx>> drop_ctx;
    {
        std::lock_guard<std::mutex> g(slot_cache_m());
        drop.swap(slot_cache());
        drop_ctx.swap(inflate_cache());
    }
    int cur = 0;
    CTO_HIP(hipGetDevice(&cur));
    for (auto& sl : drop) { CTO_HIP(hipSetDevice(sl->device)); sl.reset(); }
    for (auto& c : drop_ctx) { CTO_HIP(hipSetDevice(c->device)); c.reset(); }
    CTO_HIP(hipSetDevice(cur));
    return CTO_OK;
}
