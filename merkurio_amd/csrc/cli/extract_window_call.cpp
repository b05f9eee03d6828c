// extract_window_call.cpp -- one window of the extract window driver through the matcher: the device call (mk_extract_window /
// mk_extract_window_members / mk_extract_window_frames: its output buffers, the first guesses of their sizes, the capacity-and-repeat protocol, what comes back)
// and the host parser's path for a window the device refuses; both end with Win::kept and the text the writer needs (pack_host_text).
#include "device_abi_weak.hpp"
#include "extract_windows.hpp"

namespace cli {

using Side = xw::Side;
using Win = xw::Win;

struct WindowExtract::Impl::Call {  // the arguments of one window's device call, across its attempts
    mk_window_source src[2];
    mk_window_members mem[2];
    bool use_members = false, any_bgzf = false;
    uint64_t cap_text = 0, rec_cap = 0;
    mk_window_front front;  // (an open window)
    Call() {
        memset(&front, 0, sizeof(front));
        memset(src, 0, sizeof(src));
        memset(mem, 0, sizeof(mem));
    }
};

// contiguous text of a side on the host: head ++ body (BGZF members inflated by zlib, device text read back)
void WindowExtract::Impl::side_text(Side &S, std::vector<char> &out) {
    out.resize(S.head.size() + S.body_bytes());
    if (!S.head.empty()) memcpy(out.data(), S.head.data(), S.head.size());
    if (S.has_body()) S.from->body_to_host(S, out.data() + S.head.size());
}

// a window the device did not take: parsed by the host reader's code (which words the reference's errors), scanned in batches
void WindowExtract::Impl::host_window(Win &W, mk_matcher *m) {
    W.by_host = true;
    uint64_t n = ~0ull;
    uint64_t stop[2] = {0, 0};
    for (int i = 0; i < n_in; ++i) {
        Side &S = W.side[i];
        Side::Result &R = S.out;
        side_text(S, R.text);
        R.parsed.fastq = fastq;
        R.parsed.data = R.text.data();
        R.parsed.data_n = R.text.size();
        R.parsed.recs.clear();
        stop[i] = R.parsed.parse_span_partial(0, R.text.size(), !S.ends);
        n = std::min<uint64_t>(n, R.parsed.recs.size());
    }
    for (int i = 0; i < n_in; ++i) {
        Side::Result &R = W.side[i].out;
        // the text behind record n - 1 is the tail (the marker of record n sits one byte in front of its id)
        const uint64_t cut = n < R.parsed.recs.size() ? R.parsed.recs[n].id_b - 1 : stop[i];
        R.tail.assign(R.text.begin() + (ptrdiff_t)cut, R.text.end());
        // (what is left behind the last record of an input that has ended can only be blank lines)
        if (W.side[i].ends && n == R.parsed.recs.size()) R.tail.clear();
        R.parsed.recs.resize(n);
        R.n_used = cut;
    }
    W.n_rec = n;
    W.keep.assign(n, 0);
    W.rows.clear();
    W.n_rows = 0;
    memset(&W.cb, 0, sizeof(W.cb));
    W.cnt.assign(pats->list.size(), 0);
    const FastxFile &p1 = W.side[0].out.parsed, &p2 = W.side[1].out.parsed;
    std::vector<uint8_t> s1, s2;
    std::vector<uint64_t> o1, o2;
    std::vector<mk_row> rows(4096);
    for (size_t b0 = 0; b0 < n;) {
        size_t b1 = b0;
        uint64_t bytes = 0;
        while (b1 < n && (bytes < batch_bytes || b1 == b0)) {
            bytes += p1.raw_len(b1) + (n_in == 2 ? p2.raw_len(b1) : 0);
            ++b1;
        }
        p1.gather(b0, b1, s1, o1);
        if (n_in == 2) p2.gather(b0, b1, s2, o2);
        const uint64_t nb = b1 - b0;
        uint64_t n_rows = 0;
        for (;;) {
            mk_counters cb;
            memset(&cb, 0, sizeof(cb));
            std::vector<uint32_t> cnt_b(W.cnt.size(), 0);
            const int rc = n_in == 2 ? mk_extract_paired(m, s1.data(), o1.data(), nb, s2.data(), o2.data(), nb, lg->active, a.invert_match,
                                                         W.keep.data() + b0, rows.data(), rows.size(), &n_rows, &cb, cnt_b.data())
                                     : mk_extract_single(m, s1.data(), o1.data(), nb, lg->active, a.invert_match, W.keep.data() + b0, rows.data(),
                                                         rows.size(), &n_rows, &cb, cnt_b.data());
            if (rc == MK_E_CAPACITY && n_rows > rows.size()) {
                rows.resize(n_rows);
                continue;
            }
            mk_check(rc, "Error during matching");
            add_counters(W.cb, cb);
            add_counts(W.cnt, cnt_b);
            break;
        }
        if (lg->active)
            for (uint64_t r = 0; r < n_rows; ++r) {
                mk_row row = rows[r];
                row.rec += b0;
                W.rows.push_back(row);
            }
        b0 = b1;
    }
    W.n_rows = W.rows.size();
    W.index_kept();
}

// the inputs of every side, and per side the buffers for what has to come back of its text; -> the largest window text of a side
uint64_t WindowExtract::Impl::bind_outputs(Win &W, Call &c) {
    for (int i = 0; i < n_in; ++i) {
        Side &S = W.side[i];
        Side::Result &R = S.out;
        mk_window_source &Q = c.src[i];
        Q.head = (const uint8_t *)S.head.data(), Q.n_head = S.head.size();
        if (!S.grp.empty()) {
            Q.bgzf = in[i].s.source().file_bytes(), Q.n_bgzf = in[i].s.source().file_size();
            Q.members = S.grp.data(), Q.n_members = S.grp.size();
            c.any_bgzf = true;
        } else if (S.n_dev_body) {
            Q.device_text = S.dev_body, Q.n_device_text = S.n_dev_body;
        } else {
            Q.text = (const uint8_t *)S.body, Q.n_text = S.n_body;
        }
        Q.ends_at_record = S.ends ? 1 : 0;
        const uint64_t n_text = S.head.size() + S.body_bytes();
        c.cap_text = std::max(c.cap_text, n_text);
        if (!S.on_device) continue;  // (the host holds this text)
        // the host never sees this text: what it needs of it comes back -- with members only the tail
        if (!c.use_members && whole_text) {
            R.text.resize(n_text + 16);
            Q.all = (uint8_t *)R.text.data(), Q.all_cap = R.text.size();
            R.layout = Side::Result::WHOLE;
        } else if (!c.use_members) {
            R.text.resize(std::max<uint64_t>(1u << 20, std::min<uint64_t>(n_text, std::max<uint64_t>(64u << 20, n_text / 8))));
            Q.kept = (uint8_t *)R.text.data(), Q.kept_cap = R.text.size();
            R.layout = Side::Result::PACKED_KEPT;
        }
        R.tail.resize(std::max<size_t>(R.tail.size(), 1u << 20));
        Q.tail = (uint8_t *)R.tail.data(), Q.tail_cap = R.tail.size();
    }
    return c.cap_text;
}

// the members' and the ids' buffers are guessed, and a wrong guess is dear: their needs are known only after the scan, the gather and
// the deflate, so MK_E_CAPACITY means the whole window is processed once more.  Under -v nearly everything is kept: the written
// text's bound (a record grows by three line-end bytes at most), every member stored (every frame's block raw).  Otherwise the share of its window's text that
// the last window needed, an eighth added -- the first window is small, the ones behind it 16 times its size --, and never less than
// the text a window may come back as (anything below --z-members-from, or the bound)
void WindowExtract::Impl::guess_member_buffers(Win &W, Call &c) {
    const uint64_t bound = c.cap_text + 3 * c.rec_cap + 64;
    const uint64_t share = members_share_seen.load(), share_ids = ids_share_seen.load();
    const uint64_t stored = a.zstd_output ? bound + 16 * (bound / MK_ZSTD_CUT_GRID + 2) : bound + 31 * (bound / MK_BGZF_CUT_GRID + 1);
    uint64_t guess = a.invert_match ? stored : ((c.cap_text >> 10) + 1) * (share + (share >> 3));
    guess = std::max<uint64_t>(guess, std::min<uint64_t>(a.z_members_from, bound));
    for (int i = 0; i < n_in; ++i) {
        W.side[i].out.text.resize(std::max<uint64_t>(1u << 20, guess));
        if (lg->active) W.side[i].out.ids.resize(std::max<uint64_t>(1u << 16, ((c.cap_text >> 10) + 1) * (share_ids + (share_ids >> 3))));
    }
}

// after MK_E_CAPACITY: the call states every need -- grows what was too small; false: nothing was
bool WindowExtract::Impl::grow_named(Win &W, Call &c) {
    bool grown = false;
    if (W.n_rec > c.rec_cap) c.rec_cap = W.n_rec + W.n_rec / 16, grown = true, rec_cap_seen = std::max<uint64_t>(rec_cap_seen.load(), c.rec_cap);
    if (W.n_rows > W.rows.size()) W.rows.resize(W.n_rows), grown = true;
    if (W.open && c.front.n_front > c.front.front_cap) W.front.resize(c.front.n_front + (1u << 16)), grown = true;
    for (int i = 0; i < n_in; ++i) {
        Side::Result &R = W.side[i].out;
        mk_window_source &Q = c.src[i];
        if (Q.tail && Q.n_tail > Q.tail_cap) {
            R.tail.resize(Q.n_tail + (1u << 16));
            Q.tail = (uint8_t *)R.tail.data(), Q.tail_cap = R.tail.size();
            grown = true;
        }
        if (Q.kept && Q.n_kept_bytes > Q.kept_cap) {
            R.text.resize(Q.n_kept_bytes + (Q.n_kept_bytes >> 3));
            Q.kept = (uint8_t *)R.text.data(), Q.kept_cap = R.text.size();
            grown = true;
        }
        bool again = false;
        if (c.use_members && c.mem[i].n_member_bytes > c.mem[i].members_cap) R.text.resize(c.mem[i].n_member_bytes), again = true;
        if (c.use_members && c.mem[i].n_id_bytes > c.mem[i].ids_cap) R.ids.resize(c.mem[i].n_id_bytes + (c.mem[i].n_id_bytes >> 3)), again = true;
        if (again) grown = true, ++z_repeats;
    }
    return grown;
}

// the results of a call that took the window: sizes, tails, the kept-record index, and the text the writer will need
void WindowExtract::Impl::collect(Win &W, Call &c, mk_codec *codec) {
    if (c.use_members) {
        if (codec) {  // (frames: no upload, and the cut kernel is timed with the deflate -- z_ms[1] stays 0)
            float ms3[3] = {0, 0, 0};
            if (a.zstd_output) (void)mk_zstd_deflate_info(codec, nullptr, nullptr, ms3), ms3[0] = 0;
            else (void)mk_codec_cut_times(codec, nullptr, ms3);
            for (int k = 0; k < 3; ++k) W.z_ms[k + 1] = ms3[k];
        }
        uint64_t most = 0, most_ids = 0;
        for (int i = 0; i < n_in; ++i) {
            most = std::max<uint64_t>(most, c.mem[i].n_member_bytes);
            most_ids = std::max<uint64_t>(most_ids, c.mem[i].n_id_bytes);
            W.z_ms[0] += c.mem[i].written_ms;
        }
        members_share_seen = most / ((c.cap_text >> 10) + 1) + 1;
        ids_share_seen = most_ids / ((c.cap_text >> 10) + 1) + 1;
    }
    W.index_kept();
    for (int i = 0; i < n_in; ++i) {
        Side &S = W.side[i];
        Side::Result &R = S.out;
        const mk_window_source &Q = c.src[i];
        R.n_window = Q.n_window, R.n_used = Q.n_used;
        R.rec_start.resize(W.n_rec + 1);
        if (c.use_members) {
            R.layout = c.mem[i].as_text ? Side::Result::WRITTEN : Side::Result::MEMBERS;
            R.text.resize(c.mem[i].n_member_bytes);
            R.ids.resize(c.mem[i].n_id_bytes);
            R.id_end.resize(lg->active ? c.mem[i].n_kept : 0);
            R.n_members = c.mem[i].n_members;
        }
        if (S.on_device) {
            R.tail.resize(Q.n_tail);
            if (R.layout == Side::Result::PACKED_KEPT) R.text.resize(Q.n_kept_bytes);
            if (R.layout == Side::Result::WHOLE) R.text.resize(Q.n_window);
        } else {  // the host holds this text: the tail is the rest of head ++ body
            R.tail.clear();
            const uint64_t nh = S.head.size();
            if (R.n_used < nh) R.tail.insert(R.tail.end(), S.head.begin() + (ptrdiff_t)R.n_used, S.head.end());
            const uint64_t from = R.n_used > nh ? R.n_used - nh : 0;
            if (from < S.n_body) R.tail.insert(R.tail.end(), S.body + from, S.body + S.n_body);
            // ... and what the writer will need of it -- the kept records (all of it when the rows name records that are not
            // kept) -- is copied out here, so that the page-locked buffer goes back to the reader now, not after the write-out
            if (!c.use_members) pack_host_text(W, S);
        }
    }
}

void WindowExtract::Impl::device_window(Win &W, mk_matcher *m, mk_codec *codec) {
    // (-z / --zstd-output: a window whose written form the device refuses, *status = 2, is called once more for its kept records as
    // stored text)
    for (bool use_members = z_members;; use_members = false) {
        Call c;
        c.use_members = use_members;
        if (bind_outputs(W, c) >= 0xFFFFFFF0ull) {
            if (W.open || W.probe) {  // (the host parser reads from a record start: the chained re-run's business)
                W.refused = true;
                return;
            }
            return host_window(W, m);
        }  // (a FASTA record of 4 GiB or more: the host path's own limits apply)
        // (a guess the call corrects: for rec_cap MK_E_CAPACITY comes back before anything is scanned)
        c.rec_cap = std::max<uint64_t>(rec_cap_seen.load(), c.cap_text / (fastq ? 192 : 1024) + 16);
        W.rows.resize(std::max<size_t>(W.rows.size(), 4096));
        W.cnt.assign(pats->list.size(), 0);
        if (use_members) guess_member_buffers(W, c);
        uint32_t status = 0;
        for (int attempt = 0;; ++attempt) {
            for (int i = 0; i < n_in; ++i) {
                Side::Result &R = W.side[i].out;
                R.rec_start.resize(c.rec_cap + 1);
                c.src[i].rec_start = R.rec_start.data();
                if (!use_members) continue;
                if (lg->active) R.id_end.resize(c.rec_cap);
                c.mem[i].members = (uint8_t *)R.text.data(), c.mem[i].members_cap = R.text.size();
                c.mem[i].ids = (uint8_t *)R.ids.data(), c.mem[i].ids_cap = R.ids.size(), c.mem[i].id_end = R.id_end.data();
                c.mem[i].text_below = a.z_members_from;
            }
            if (W.keep.size() < c.rec_cap) W.keep.resize(c.rec_cap);
            if (W.open) {
                if (W.front.empty()) W.front.resize(1u << 20);
                c.front.front = (uint8_t *)W.front.data(), c.front.front_cap = W.front.size();
            }
            memset(&W.cb, 0, sizeof(W.cb));
            std::fill(W.cnt.begin(), W.cnt.end(), 0);
            const uint32_t format = fastq ? MK_TEXT_FASTQ : MK_TEXT_FASTA;
            const auto packed = a.zstd_output ? mk_extract_window_frames : mk_extract_window_members;
            const int rc = W.open ? mk_extract_window_open(m, c.any_bgzf ? codec : nullptr, format, 1, c.src, lg->active, a.invert_match, c.rec_cap, &W.n_rec,
                                                           W.keep.data(), W.rows.data(), W.rows.size(), &W.n_rows, &W.cb, W.cnt.data(), &status, &c.front)
                           : use_members ? packed(m, codec, format, (uint32_t)n_in, c.src, c.mem, lg->active, a.invert_match, c.rec_cap,
                                                &W.n_rec, W.keep.data(), W.rows.data(), W.rows.size(), &W.n_rows, &W.cb, W.cnt.data(), &status)
                                       : mk_extract_window(m, c.any_bgzf ? codec : nullptr, format, (uint32_t)n_in, c.src, lg->active, a.invert_match, c.rec_cap,
                                                           &W.n_rec, W.keep.data(), W.rows.data(), W.rows.size(), &W.n_rows, &W.cb, W.cnt.data(), &status);
            if (rc == MK_E_CAPACITY && attempt < 8 && grow_named(W, c)) continue;  // once more with what was too small grown
            if (rc == MK_E_CORRUPT) bail("Error while decompressing " + in[c.src[1].n_members && !c.src[0].n_members ? 1 : 0].path);
            if ((rc == MK_E_UNSUPPORTED || rc == MK_E_NOMEM) && (W.open || W.probe)) {  // (the chained re-run takes what follows from it)
                W.refused = true;
                return;
            }
            if (rc == MK_E_UNSUPPORTED || rc == MK_E_NOMEM) {
                // too much for the device in one piece (a pair of windows above 2 GiB under BNDMq; no memory for the window): the
                // host path takes this window in batches, and BGZF windows shrink from here on
                if (rc == MK_E_NOMEM) {
                    std::lock_guard<std::mutex> lk(gate.mu);
                    bgzf_target = std::max<uint64_t>(64ull << 20, bgzf_target / 2);
                }
                return host_window(W, m);
            }
            mk_check(rc, "Error during matching");
            break;
        }
        if (status == 2 && use_members) {
            for (int i = 0; i < n_in; ++i) W.side[i].out.text.clear(), W.side[i].out.ids.clear(), W.side[i].out.id_end.clear();
            continue;
        }
        if (status != 0 && (W.open || W.probe)) {  // no start, or not what the device takes from there: the guess is disproved
            W.refused = true;
            return;
        }
        if (status != 0) return host_window(W, m);
        if (W.open) W.front.resize(c.front.n_front);
        return collect(W, c, codec);
    }
}

// S.out.text = the kept records of a host-held window back to back (layout PACKED_KEPT), or its whole text (WHOLE)
void WindowExtract::Impl::pack_host_text(const Win &W, Side &S) {
    Side::Result &R = S.out;
    const uint64_t nh = S.head.size();
    auto piece = [&](uint64_t b, uint64_t e, char *dst) {  // text[b, e) of head ++ body
        if (b < nh) {
            const uint64_t k = std::min(e, nh) - b;
            memcpy(dst, S.head.data() + b, (size_t)k);
            dst += k, b += k;
        }
        if (b < e) memcpy(dst, S.body + (b - nh), (size_t)(e - b));
    };
    if (whole_text) {
        R.text.resize(R.n_used);
        const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), (size_t)(R.n_used >> 22) + 1));
        run_threads(T, [&](size_t t) { piece(R.n_used * t / T, R.n_used * (t + 1) / T, R.text.data() + R.n_used * t / T); });
        R.layout = Side::Result::WHOLE;
        return;
    }
    std::vector<uint64_t> at;
    uint64_t total = 0;
    for (uint64_t r : W.kept) {
        at.push_back(total);
        total += R.rec_start[r + 1] - R.rec_start[r];
    }
    R.text.resize(total);
    const size_t T = std::max<size_t>(1, std::min<size_t>(io_threads(), (size_t)(total >> 22) + 1));
    run_threads(T, [&](size_t t) {
        for (size_t q = W.kept.size() * t / T; q < W.kept.size() * (t + 1) / T; ++q) piece(R.rec_start[W.kept[q]], R.rec_start[W.kept[q] + 1], R.text.data() + at[q]);
    });
    R.layout = Side::Result::PACKED_KEPT;
}

}  // namespace cli
