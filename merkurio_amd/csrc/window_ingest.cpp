// window_ingest.cpp -- text windows in: the raw bytes of a window of an input file go to the device as they are (plain text is uploaded,
// taken from an upload-ahead slot or copied from device text; BGZF members are inflated there), are indexed (line table, record tables)
// and their sequences gathered and scanned there (ingest.hip), and pieces of the text are packed for the way back.  extract_window.cpp
// and tag_windows.cpp are made of these steps (r05: FASTA, paired inputs, heads).
#include <mutex>

#include "device_loop.hpp"
#include "codec/codec_internal.h"
#include "codec/codec_kernels.h"

namespace mk {

// text of a source -> T->d_text[0, n_window): head, then the body (uploaded, taken from an upload-ahead slot, or inflated from
// BGZF members).  Enqueued on st; the caller synchronises.  A damaged member: MK_E_CORRUPT, its index in the message.
int window_assemble(mk_matcher *m, mk_codec *codec, mk_window_source &S, WindowSide &W, DeviceLoop &dl) {
    hipStream_t st = dl.st;
    int rc;
    uint64_t body = S.n_text;
    for (uint64_t i = 0; i < S.n_members; ++i) {
        const mk_bgzf_member &b = S.members[i];
        if (b.data_off > S.n_bgzf || b.data_len > S.n_bgzf - b.data_off || b.isize > 65536 || b.out_off != body - S.n_text)
            return fail(MK_E_INVALID_ARG, "mk_extract_window: member %llu lies outside its buffer or its text is not in sequence", (unsigned long long)i);
        body += b.isize;
    }
    if ((S.n_text != 0) + (S.n_members != 0) + (S.n_device_text != 0) > 1)
        return fail(MK_E_INVALID_ARG, "mk_extract_window: a source's body is plain text, BGZF members or device text -- one of them");
    body += S.n_device_text;
    W.n_window = S.n_head + body;
    S.n_window = W.n_window;
    if (W.n_window == 0) return MK_OK;
    if (W.n_window >= 0xFFFFFFF0ull) return fail(MK_E_UNSUPPORTED, "a text window must be shorter than 4 GiB (%llu bytes)", (unsigned long long)W.n_window);
    mk_matcher::TextSlot &T = *W.T;
    // a body that mk_upload_text_ahead has already sent (same pointer, same size): without a head its buffer BECOMES the text
    // buffer, with one it is copied behind the head on the device
    bool ahead = false;
    if (S.n_text) {
        std::lock_guard<std::mutex> lk(m->ahead_mu);
        for (auto &a : m->ahead) {
            if (!a.text || a.text != S.text || ahead) continue;
            if (a.n != S.n_text) {  // (another window out of the same buffer: stale)
                if (hipEventSynchronize(a.ev) != hipSuccess) return fail(MK_E_HIP, "hipEventSynchronize failed");
                a.text = nullptr;
                continue;
            }
            if (hipStreamWaitEvent(st, a.ev, 0) != hipSuccess) return fail(MK_E_HIP, "hipStreamWaitEvent failed");
            if (S.n_head == 0) {
                std::swap(T.d_text, a.d);
                std::swap(T.d_text_cap, a.cap);
            } else {
                if ((rc = ensure_device(&T.d_text, &T.d_text_cap, W.n_window + 64))) return rc;
                if (hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, a.d, S.n_text, hipMemcpyDeviceToDevice, st) != hipSuccess)
                    return fail(MK_E_HIP, "copy of the uploaded window failed");
                // (the slot may be refilled by the uploader as soon as it is marked free: let the copy out of it finish first)
                if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "copy of the uploaded window failed");
            }
            a.text = nullptr;
            ahead = true;
        }
    }
    if (!ahead && (rc = ensure_device(&T.d_text, &T.d_text_cap, W.n_window + 64))) return rc;
    if (S.n_head && hipMemcpyAsync(T.d_text, S.head, S.n_head, hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "upload of the head failed");
    if (S.n_text && !ahead && hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, S.text, S.n_text, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(MK_E_HIP, "upload of the text failed");
    if (S.n_device_text && hipMemcpyAsync((uint8_t *)T.d_text + S.n_head, S.device_text, S.n_device_text, hipMemcpyDefault, st) != hipSuccess)
        return fail(MK_E_HIP, "copy of the device text failed");
    if (S.n_members) {
        if (!codec) return fail(MK_E_INVALID_ARG, "mk_extract_window: BGZF members need a codec handle");
        if (codec->device != m->device) return fail(MK_E_INVALID_ARG, "mk_extract_window: the codec and the matcher are on different devices");
        // the members' bytes and their table go up (a fifth of the text), the text is inflated behind the head in place
        std::lock_guard<std::mutex> lock(codec->mu);
        uint64_t in_lo = S.members[0].data_off, in_hi = in_lo;
        std::vector<mkz::Member> part(S.n_members);
        for (uint64_t i = 0; i < S.n_members; ++i) {
            in_lo = std::min<uint64_t>(in_lo, S.members[i].data_off);
            in_hi = std::max<uint64_t>(in_hi, S.members[i].data_off + S.members[i].data_len);
        }
        for (uint64_t i = 0; i < S.n_members; ++i)
            part[i] = mkz::Member{S.members[i].data_off - in_lo, S.n_head + S.members[i].out_off, S.members[i].data_len, S.members[i].isize, S.members[i].crc, 0};
        const uint64_t cn = in_hi - in_lo;
        if ((rc = ensure_device(&codec->d_in, &codec->in_cap, cn + mkz::kPad)) ||
            (rc = ensure_device(&codec->d_aux, &codec->aux_cap, (S.n_members + 1) * sizeof(mkz::Member))) ||
            (rc = ensure_device(&codec->d_len, &codec->len_cap, (S.n_members + 1) * 4ull)))
            return rc;
        if (hipMemcpyAsync(codec->d_in, S.bgzf + in_lo, cn, hipMemcpyHostToDevice, st) != hipSuccess ||
            hipMemsetAsync((uint8_t *)codec->d_in + cn, 0, mkz::kPad, st) != hipSuccess ||
            hipMemcpyAsync(codec->d_aux, part.data(), S.n_members * sizeof(mkz::Member), hipMemcpyHostToDevice, st) != hipSuccess)
            return fail(MK_E_HIP, "upload of the members failed");
        if (hipStreamSynchronize(st) != hipSuccess) return fail(MK_E_HIP, "upload of the members failed");
        dl.mark(1);
        mkz::launch_inflate((const uint8_t *)codec->d_in, cn, (const mkz::Member *)codec->d_aux, (uint32_t)S.n_members, (uint8_t *)T.d_text,
                            (int32_t *)codec->d_len, codec->num_cus, st, codec->inflate_kernel);
        mkz::launch_crc_check((const uint8_t *)T.d_text, (const mkz::Member *)codec->d_aux, (uint32_t)S.n_members, (int32_t *)codec->d_len, st);
        std::vector<int32_t> st_words(S.n_members);
        if (hipGetLastError() != hipSuccess ||
            hipMemcpyAsync(st_words.data(), codec->d_len, S.n_members * 4ull, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "BGZF inflate failed");
        dl.mark(2);
        for (uint64_t i = 0; i < S.n_members; ++i)
            if (st_words[i])
                return fail(MK_E_CORRUPT, st_words[i] > 0 ? "BGZF member %llu: CRC-32 of the inflated text differs from the trailer's (status %d)"
                                                           : "BGZF member %llu does not inflate to its ISIZE (decoder status %d)",
                            (unsigned long long)i, st_words[i]);
    }
    return MK_OK;
}

// the newline count of W's text (enqueued work waited for): d_ing_a carved -- newline count per block | total | status, min, max |
// extra_bytes of the caller's behind these n_blocks + 8 words -- W.total_nl, W.last_byte and, if asked for, the first byte
int line_table(WindowSide &W, hipStream_t st, size_t extra_bytes, uint8_t *first_byte) {
    mk_matcher::TextSlot &T = *W.T;
    const uint64_t n_text = W.n_window;
    const uint8_t *d_text = (const uint8_t *)T.d_text;
    const uint32_t n_blocks = (uint32_t)((n_text + ingest_block_bytes() - 1) / ingest_block_bytes());
    if (int rc = ensure_device(&T.d_ing_a, &T.d_ing_a_cap, ((size_t)n_blocks + 8) * 4 + extra_bytes)) return rc;
    W.d_block = (uint32_t *)T.d_ing_a;
    W.d_total = W.d_block + n_blocks;
    W.d_st = W.d_total + 1;
    launch_ingest_count(d_text, n_text, W.d_block, W.d_total, st);
    if (hipMemcpyAsync(&W.total_nl, W.d_total, 4, hipMemcpyDeviceToHost, st) != hipSuccess ||
        (first_byte && hipMemcpyAsync(first_byte, d_text, 1, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipMemcpyAsync(&W.last_byte, d_text + n_text - 1, 1, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "newline count failed");
    return MK_OK;
}

// line table, whole records and their tables for the text in W.T (enqueued work waited for): W.n_avail, d_rec_start[n_avail + 1],
// FASTQ: d_seq_start / d_seq_len / W.fixed; FASTA: the sequences already lie in d_seq_out with offsets d_fa_off[n_avail + 1].
// *status = 1: this text is not what the device takes (the caller's reader decides what it is).
// open_from != nullptr: the window may begin anywhere (mk_extract_window_open) -- its first record start is found in the line table
// (mk_ingest_open_start_kernel) and the records are indexed from there; *open_from = that byte, every table stays in offsets of the
// whole text.  *status = 2: no start was found.
int window_index(mk_matcher *m, uint32_t format, bool ends_at_record, WindowSide &W, uint8_t *d_seq_out, hipStream_t st, uint32_t *status,
                 uint64_t *open_from) {
    mk_matcher::TextSlot &T = *W.T;
    int rc;
    const uint64_t n_text = W.n_window;
    const uint8_t *d_text = (const uint8_t *)T.d_text;
    const uint32_t n_blocks = (uint32_t)((n_text + ingest_block_bytes() - 1) / ingest_block_bytes());
    // (behind line_table's words: FASTA's u64 per block + 1; an open window: one more, the word its start is found in)
    uint8_t first = 0;
    if ((rc = line_table(W, st, 16 + ((size_t)n_blocks + 2 + (open_from ? 1 : 0)) * 8, &first))) return rc;
    W.d_block64 = (unsigned long long *)(((uintptr_t)(W.d_block + n_blocks + 8) + 15) & ~(uintptr_t)15);
    const uint32_t total_nl = W.total_nl;
    // an open window: the line table first (its place in d_ing_b is the same in both layouts below), then the found start
    uint64_t j0 = 0, from = 0;
    if (open_from) {
        // (room for the whole workspace now, sized as if the first line were the start: the table must not move afterwards)
        const size_t most_rec = format == MK_TEXT_FASTA ? (size_t)total_nl + 2 : (size_t)total_nl / 4 + 1;
        const size_t ws = format == MK_TEXT_FASTA ? ((size_t)total_nl + 4) * 4 + (most_rec + 2) * 4 + 16 + (most_rec + 2) * 8
                                                  : ((size_t)total_nl + 4 + 3 * (most_rec + 2) + 8) * 4 + (most_rec / ingest_scan_tile() + 2) * 8 + 64;
        if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ws))) return rc;
        unsigned long long *d_found = W.d_block64 + n_blocks + 2, found = ~0ull;
        launch_ingest_lines(d_text, n_text, W.d_block, W.d_total, (uint32_t *)T.d_ing_b, st);
        launch_ingest_open_start(d_text, n_text, (const uint32_t *)T.d_ing_b, total_nl, format == MK_TEXT_FASTA, d_found, st);
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&found, d_found, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "search for the window's first record failed");
        if (found == ~0ull) {
            *status = 2;
            return MK_OK;
        }
        j0 = found >> 32, from = found & 0xFFFFFFFFull;
        *open_from = from;
    }
    if (format == MK_TEXT_FASTA) {
        if (!open_from && first != '>') {  // blank lines or anything else in front of the first header: the host reader's business
            *status = 1;
            return MK_OK;
        }
        // line table | record starts | (u64) sequence offsets
        const size_t max_rec = (size_t)total_nl + 2;  // (a header per line at most)
        const size_t ws = ((size_t)total_nl + 4) * 4 + (max_rec + 2) * 4 + 16 + (max_rec + 2) * 8;
        if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ws))) return rc;
        W.d_line = (uint32_t *)T.d_ing_b;
        W.d_rec_start = W.d_line + total_nl + 4;
        W.d_fa_off = (unsigned long long *)(((uintptr_t)(W.d_rec_start + max_rec + 2) + 15) & ~(uintptr_t)15);
        if (!open_from) launch_ingest_lines(d_text, n_text, W.d_block, W.d_total, W.d_line, st);  // (an open window's table exists, in this very place)
        if (hipMemsetAsync(W.d_block64 + n_blocks, 0, 8, st) != hipSuccess) return fail(MK_E_HIP, "hipMemsetAsync failed");
        launch_ingest_fasta_count(d_text, n_text, W.d_block, W.d_line, W.d_block64, st, from);
        unsigned long long totals = 0;
        if (hipGetLastError() != hipSuccess || hipMemcpyAsync(&totals, W.d_block64 + n_blocks, 8, hipMemcpyDeviceToHost, st) != hipSuccess ||
            hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "FASTA indexing failed");
        const uint64_t heads = totals >> 32;
        W.seq_total = totals & 0xFFFFFFFFull;
        launch_ingest_fasta_emit(d_text, n_text, W.d_block, W.d_line, W.d_block64, d_seq_out, W.d_rec_start, W.d_fa_off, st, from);
        if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, "FASTA gather failed to launch");
        // a record is whole once the next header (or the end of the input) has been seen
        W.n_avail = ends_at_record ? heads : (heads ? heads - 1 : 0);
        W.fixed = 0;
        return MK_OK;
    }
    uint64_t n_lines = total_nl - j0;  // (an open window: the lines from the found one on)
    if (ends_at_record) {
        n_lines += W.last_byte != '\n' ? 1 : 0;
        if (n_lines % 4 != 0) {  // not whole 4-line records: the caller's reader decides what this text is
            *status = 1;
            return MK_OK;
        }
    }
    const uint64_t n_rec = n_lines / 4;
    W.n_avail = n_rec;
    // workspace: line starts | record starts (+1) | sequence starts | sequence lengths | tile sums
    const size_t n_tiles = n_rec / ingest_scan_tile() + 2;
    const size_t ws = ((size_t)total_nl + 4 + 3 * (n_rec + 2) + 8) * 4 + n_tiles * 8 + 64;
    if ((rc = ensure_device(&T.d_ing_b, &T.d_ing_b_cap, ws))) return rc;
    uint32_t *const d_line0 = (uint32_t *)T.d_ing_b;
    W.d_line = d_line0 + j0;  // line 4 r + k of the table is line k of record r
    W.d_rec_start = d_line0 + total_nl + 4;
    W.d_seq_start = W.d_rec_start + n_rec + 2;
    W.d_seq_len = W.d_seq_start + n_rec + 2;
    W.d_tile = (unsigned long long *)(((uintptr_t)(W.d_seq_len + n_rec + 2) + 15) & ~(uintptr_t)15);
    const uint32_t st_init[3] = {0u, 0xFFFFFFFFu, 0u};
    if (hipMemcpyAsync(W.d_st, st_init, sizeof(st_init), hipMemcpyHostToDevice, st) != hipSuccess) return fail(MK_E_HIP, "copy failed");
    if (open_from) launch_ingest_index(d_text, n_text, W.d_line, n_rec, W.d_rec_start, W.d_seq_start, W.d_seq_len, W.d_st, st);  // (the table exists)
    else launch_ingest_records(d_text, n_text, W.d_block, W.d_total, W.d_line, n_rec, W.d_rec_start, W.d_seq_start, W.d_seq_len, W.d_st, st);
    uint32_t st_host[3] = {0, 0, 0};
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(st_host, W.d_st, sizeof(st_host), hipMemcpyDeviceToHost, st) != hipSuccess ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "record indexing failed");
    if (st_host[0]) {  // some record is not '@' / sequence / '+' / quality of equal length
        *status = 1;
        return MK_OK;
    }
    W.fixed = (n_rec && st_host[1] == st_host[2] && st_host[1] > 0) ? st_host[1] : 0;
    return MK_OK;
}

// the sequences of W's first n records -> the scan buffer, scanned: flags (host + m->d_flags), tuples in m->d_hits (dl.found), *n_seq
// sequence bytes.  FASTQ / BAM / SAM are gathered by W.d_seq_start / W.d_seq_len (W.fixed > 0: all of that length) in the way their
// form asks for; FASTA's were compacted by the index step.
int scan_sequences(mk_matcher *m, const WindowSide &W, uint64_t n, SeqForm form, DeviceLoop &dl, uint32_t mode, uint8_t *flags, uint64_t *flagged,
                   uint64_t *n_seq) {
    hipStream_t st = dl.st;
    const uint32_t fixed = W.fixed;
    unsigned long long total = (unsigned long long)n * fixed;
    int rc;
    if ((rc = ensure_device((void **)&m->d_flags, &m->d_flags_cap, n + 8)) || (rc = ensure_device((void **)&m->d_off, &m->d_off_cap, (n + 1) * sizeof(uint64_t))))
        return rc;
    if (W.d_fa_off) {  // FASTA: the offsets of the compacted sequences become the batch's
        if (hipMemcpyAsync(m->d_off, W.d_fa_off, (n + 1) * 8, hipMemcpyDeviceToDevice, st) != hipSuccess ||
            hipMemcpyAsync(&total, W.d_fa_off + n, 8, hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess)
            return fail(MK_E_HIP, "copy of the sequence offsets failed");
        *n_seq = total;
        // (one record of 4 GiB or more cannot be addressed by mk_hit.pos, as mk_scan_batch refuses it.)  The sequences lie in the
        // slot's own buffer: it stands in for the scan buffer for this scan.
        mk_matcher::TextSlot &T = *W.T;
        void *seq = m->d_seq;
        size_t cap = m->d_seq_cap;
        m->d_seq = (uint8_t *)T.d_fa_seq, m->d_seq_cap = T.d_fa_seq_cap;
        rc = dl.scan_resident(total, n, mode, 0, flags, flagged);
        T.d_fa_seq = m->d_seq, T.d_fa_seq_cap = m->d_seq_cap;
        m->d_seq = (uint8_t *)seq, m->d_seq_cap = cap;
        return rc;
    }
    if (!fixed && (rc = scan_offsets(W.d_seq_len, n, W.d_tile, (unsigned long long *)m->d_off, st, &total, "offset scan failed"))) return rc;
    *n_seq = total;
    if ((rc = ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64))) return rc;
    if (form == kSeqBam) launch_bam_unpack((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    else if (form == kSeqSam) launch_sam_gather((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    else launch_ingest_gather((const uint8_t *)W.T->d_text, W.d_seq_start, W.d_seq_len, (const unsigned long long *)m->d_off, fixed, n, m->d_seq, st);
    if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, form == kSeqPlain ? "ingest kernels failed to launch" : "sequence unpacking failed to launch");
    return dl.scan_resident(total, n, mode, fixed, flags, flagged);
}

// ---- pieces of the window's text, back to back in m->d_seq (the scan buffer has done its work when anything is packed): the lengths
// are the caller's, scan_offsets into m->d_off says where each piece goes and what they take -- the caller checks that against its
// capacity -- then room, gather and download.  pad: bytes the caller wants behind the pieces.
int pack_room(mk_matcher *m, unsigned long long total, size_t pad) { return ensure_device((void **)&m->d_seq, &m->d_seq_cap, total + 64 + pad); }

// piece r = text[d_start[r], + d_len[r]) (pieces of big_from bytes and more are left to the caller)
int pack_gather(mk_matcher *m, const WindowSide &W, const uint32_t *d_start, const uint32_t *d_len, uint64_t n, unsigned long long total, size_t pad,
                uint32_t big_from, hipStream_t st, const char *what) {
    if (int rc = pack_room(m, total, pad)) return rc;
    launch_ingest_gather((const uint8_t *)W.T->d_text, d_start, d_len, (const unsigned long long *)m->d_off, 0, n, m->d_seq, st, big_from);
    if (hipGetLastError() != hipSuccess) return fail(MK_E_HIP, "%s", what);
    return MK_OK;
}

// the packed bytes -> dst (enqueued work waited for)
int pack_download(mk_matcher *m, void *dst, unsigned long long total, hipStream_t st, const char *what) {
    if (hipGetLastError() != hipSuccess || (total && hipMemcpyAsync(dst, m->d_seq, total, hipMemcpyDeviceToHost, st) != hipSuccess) ||
        hipStreamSynchronize(st) != hipSuccess)
        return fail(MK_E_HIP, "%s", what);
    return MK_OK;
}

}  // namespace mk

using namespace mk;

extern "C" {

int mk_upload_text_ahead(mk_matcher *m, const uint8_t *text, uint64_t n_text) {
    if (!m || (n_text && !text)) return fail(MK_E_INVALID_ARG, "null argument");
    if (n_text == 0 || n_text >= 0xFFFFFFF0ull) return MK_OK;  // (nothing to do / the call itself will refuse it)
    MK_ABI_BEGIN
    if (hipSetDevice(m->device) != hipSuccess) return fail(MK_E_HIP, "hipSetDevice failed");
    std::lock_guard<std::mutex> lk(m->ahead_mu);
    if (!m->stream_ahead && hipStreamCreateWithFlags(&m->stream_ahead, hipStreamNonBlocking) != hipSuccess)
        return fail(MK_E_HIP, "hipStreamCreate failed");
    mk_matcher::AheadSlot *slot = nullptr;
    // a slot that still holds an earlier window from this very buffer is stale (the host did not come back for it and is now
    // refilling the buffer): its copy must have finished reading before the new bytes are trusted -- the caller has of course
    // already overwritten them, so all that is left to do is to wait and take the slot over
    for (auto &a : m->ahead)
        if (a.text == text) {
            if (hipEventSynchronize(a.ev) != hipSuccess) return fail(MK_E_HIP, "hipEventSynchronize failed");
            a.text = nullptr;
            slot = &a;
        }
    for (auto &a : m->ahead)
        if (!a.text && !slot) slot = &a;
    if (!slot) return MK_OK;  // every slot waits already: this window will upload itself
    if (!slot->ev && hipEventCreateWithFlags(&slot->ev, hipEventDisableTiming) != hipSuccess) return fail(MK_E_HIP, "hipEventCreate failed");
    int rc = ensure_device(&slot->d, &slot->cap, n_text + 64);
    if (rc) return rc;
    if (hipMemcpyAsync(slot->d, text, n_text, hipMemcpyHostToDevice, m->stream_ahead) != hipSuccess ||
        hipEventRecord(slot->ev, m->stream_ahead) != hipSuccess)
        return fail(MK_E_HIP, "upload of the next text window failed");
    slot->text = text;
    slot->n = n_text;
    return MK_OK;
    MK_ABI_END
}

}  // extern "C"
