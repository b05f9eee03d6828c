#include "bam_out.hpp"

#include <zlib.h>

#include <algorithm>
#include <chrono>
#include <cstring>

#include "bam_text.hpp"
#include "device_abi_weak.hpp"

namespace cli {

BamWriter::~BamWriter() {
    try {
        close();  // (the command closes the writer itself: an error surfaces there, not here)
    } catch (...) {
    }
}

void BamWriter::use_device(int device) { device_ = mk_bgzf_deflate_pieces ? device : -1; }

constexpr size_t kBgzfBlock = 0xff00;

void BamWriter::put(const void *p, size_t n) {  // small writes (header, single records) share an open piece
    if (pieces.empty() || pieces.back().size() + n > pieces.back().capacity()) {
        pieces.emplace_back();
        pieces.back().reserve(std::max<size_t>(n, 1u << 20));
    }
    pieces.back().insert(pieces.back().end(), (const uint8_t *)p, (const uint8_t *)p + n);
    pieces_bytes += n;
    if (pieces_bytes >= (run_members + 1) * kBgzfBlock) flush(false);
}

std::vector<uint8_t> BamWriter::take_buffer() {
    std::lock_guard<std::mutex> lk(mu_);
    if (free_.empty()) return {};
    std::vector<uint8_t> b = std::move(free_.back());
    free_.pop_back();
    return b;
}

void BamWriter::put_encoded(std::vector<uint8_t> &&bytes) {
    if (bytes.empty()) return;
    pieces_bytes += bytes.size();
    pieces.push_back(std::move(bytes));
    if (pieces_bytes >= (run_members + 1) * kBgzfBlock) flush(false);
}

constexpr size_t kMaxQueuedRuns = 6;

HostBuffer BamWriter::take_raw_buffer(size_t min_size) {
    HostBuffer b;
    {
        std::lock_guard<std::mutex> lk(mu_);
        for (size_t k = 0; k < free_raw_.size(); ++k)
            if (free_raw_[k].cap >= min_size || k + 1 == free_raw_.size()) {
                b = std::move(free_raw_[k]);
                free_raw_.erase(free_raw_.begin() + k);
                break;
            }
    }
    if (!b.grow(min_size, 0, true)) bail("Error writing BAM file: out of memory");
    return b;
}

void BamWriter::enqueue(Run &&run) {
    std::unique_lock<std::mutex> lk(mu_);
    if (failed_) std::rethrow_exception(failed_);
    if (!writer_.joinable()) writer_ = std::thread([this] { writer_loop(); });
    cv_.wait(lk, [&] { return queue_.size() < kMaxQueuedRuns; });
    queue_.push_back(std::move(run));
    lk.unlock();
    cv_.notify_all();
}

void BamWriter::put_members(HostBuffer &&buffer, size_t used) {
    Run run;
    run.raw = true;
    run.raw_buf = std::move(buffer);
    run.raw_used = used;
    flush(true);
    enqueue(std::move(run));
}

// one BGZF member: gzip header with the BC extra field, raw deflate, crc32, isize
void bgzf_compress(const uint8_t *in, size_t n, std::vector<uint8_t> &out) {
    out.resize(n + n / 8 + 1024);
    z_stream z;
    memset(&z, 0, sizeof(z));
    if (deflateInit2(&z, 6, Z_DEFLATED, -15, 8, Z_DEFAULT_STRATEGY) != Z_OK) bail("Error writing BAM file: zlib init failed");
    z.next_in = const_cast<Bytef *>(in);
    z.avail_in = (uInt)n;
    z.next_out = out.data() + 18;
    z.avail_out = (uInt)(out.size() - 26);
    if (deflate(&z, Z_FINISH) != Z_STREAM_END) bail("Error writing BAM file: deflate failed");
    const size_t clen = z.total_out;
    deflateEnd(&z);
    static const uint8_t hdr[16] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0};
    memcpy(out.data(), hdr, 16);
    const uint16_t bsize = (uint16_t)(clen + 25);  // total block size - 1
    memcpy(out.data() + 16, &bsize, 2);
    const uint32_t crc = (uint32_t)crc32(crc32(0, nullptr, 0), in, (uInt)n);
    const uint32_t isize = (uint32_t)n;
    memcpy(out.data() + 18 + clen, &crc, 4);
    memcpy(out.data() + 22 + clen, &isize, 4);
    out.resize(clen + 26);
}

void BamWriter::writer_loop() {
    for (;;) {
        Run run;
        {
            std::unique_lock<std::mutex> lk(mu_);
            cv_.wait(lk, [&] { return !queue_.empty() || closing_; });
            if (queue_.empty()) return;
            run = std::move(queue_.front());
            queue_.pop_front();
            busy_ = true;
        }
        cv_.notify_all();
        try {
            if (run.raw) {
                const bool ok = failed_ || fwrite(run.raw_buf.p, 1, run.raw_used, f) == run.raw_used;
                {
                    std::lock_guard<std::mutex> lk(mu_);
                    if (free_raw_.size() < 4) free_raw_.push_back(std::move(run.raw_buf));
                }
                run.raw_buf.reset();  // (a fifth spare is freed now, not kept to the end of the process)
                if (!ok) bail("Error writing BAM file");
            } else if (!failed_) {
                compress_and_write(run);
            }
        } catch (...) {
            std::lock_guard<std::mutex> lk(mu_);
            if (!failed_) failed_ = std::current_exception();
        }
        {
            std::lock_guard<std::mutex> lk(mu_);
            busy_ = false;
        }
        cv_.notify_all();
    }
}

// whole members of the stream so far (all of it at close) go to the writer thread; the bytes behind the last whole
// member -- less than one member -- stay, as the first piece of what follows
void BamWriter::flush(bool all) {
    const size_t take = all ? pieces_bytes : pieces_bytes / kBgzfBlock * kBgzfBlock;
    if (!take) return;
    Run run;
    std::vector<uint8_t> rest;
    size_t at = 0;
    for (auto &p : pieces) {
        if (at + p.size() <= take) {
            at += p.size();
            run.push_back(std::move(p));
        } else {
            const size_t keep = at < take ? take - at : 0;  // bytes of this piece that belong to the run
            rest.insert(rest.end(), p.begin() + keep, p.end());
            at += p.size();
            if (keep) {
                p.resize(keep);
                run.push_back(std::move(p));
            }
        }
    }
    pieces.clear();
    pieces_bytes = rest.size();
    if (!rest.empty()) pieces.push_back(std::move(rest));
    enqueue(std::move(run));
}

void BamWriter::compress_and_write(Run &run_) {
    const auto t0 = std::chrono::steady_clock::now();
    size_t total = 0;
    for (auto &p : run_) total += p.size();
    if (device_ >= 0) {  // the device codec: every member of the run in one call, the pieces joined on the device
        if (!codec_) {
            mk_codec *c = nullptr;
            if (mk_codec_create(device_, &c) != MK_OK) bail(std::string("Error writing BAM file: ") + mk_last_error());
            codec_ = c;
        }
        std::vector<const uint8_t *> ptr(run_.size());
        std::vector<uint64_t> len(run_.size());
        for (size_t k = 0; k < run_.size(); ++k) ptr[k] = run_[k].data(), len[k] = run_[k].size();
        z_.resize(mk_bgzf_deflate_bound(total, (uint32_t)kBgzfBlock));
        uint64_t zn = 0;
        if (mk_bgzf_deflate_pieces((mk_codec *)codec_, ptr.data(), len.data(), ptr.size(), (uint32_t)kBgzfBlock, z_.data(), z_.size(), &zn) != MK_OK)
            bail(std::string("Error writing BAM file: ") + mk_last_error());
        deflate_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (fwrite(z_.data(), 1, zn, f) != zn) bail("Error writing BAM file");
        {
            std::lock_guard<std::mutex> lk(mu_);
            for (auto &p : run_)
                if (p.capacity() >= (1u << 20) && free_.size() < 64) {
                    p.clear();
                    free_.push_back(std::move(p));
                }
        }
        run_.clear();
        return;
    }
    // zlib on every host thread (deflate is the slow side of BAM output: ~50 MB/s per core); members written in order
    flat_.clear();
    flat_.reserve(total);
    for (auto &p : run_) flat_.insert(flat_.end(), p.begin(), p.end());
    run_.clear();
    const std::vector<uint8_t> &run = flat_;
    const size_t blocks = (run.size() + kBgzfBlock - 1) / kBgzfBlock;
    std::vector<std::vector<uint8_t>> outs(blocks);
    const size_t T = std::min<size_t>(io_threads(), blocks);
    run_threads(T, [&](size_t t) {
        for (size_t i = t; i < blocks; i += T) bgzf_compress(run.data() + i * kBgzfBlock, std::min(kBgzfBlock, run.size() - i * kBgzfBlock), outs[i]);
    });
    deflate_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    for (auto &o : outs)
        if (fwrite(o.data(), 1, o.size(), f) != o.size()) bail("Error writing BAM file");
}

void BamWriter::open(const std::string &path, const std::string &header_text, const std::vector<std::string> *names,
                     const std::vector<uint32_t> *lens) {
    f = fopen(path.c_str(), "wb");
    if (!f) bail("Error writing BAM file: " + path);
    std::vector<uint32_t> ref_len;
    if (names && lens) {
        ref_names = *names;
        ref_len = *lens;
    }
    size_t b = names && lens ? header_text.size() : 0;
    while (b < header_text.size()) {  // @SQ SN:name LN:len
        size_t e = header_text.find('\n', b);
        if (e == std::string::npos) e = header_text.size();
        const std::string ln = header_text.substr(b, e - b);
        if (ln.rfind("@SQ", 0) == 0) {
            std::string sn;
            uint32_t lnv = 0;
            size_t q = 0;
            while (q < ln.size()) {
                size_t t = ln.find('\t', q);
                if (t == std::string::npos) t = ln.size();
                if (ln.compare(q, 3, "SN:") == 0) sn = ln.substr(q + 3, t - q - 3);
                if (ln.compare(q, 3, "LN:") == 0) lnv = (uint32_t)strtoul(ln.c_str() + q + 3, nullptr, 10);
                q = t + 1;
            }
            ref_names.push_back(sn);
            ref_len.push_back(lnv);
        }
        b = e + 1;
    }
    put("BAM\1", 4);
    const int32_t l_text = (int32_t)header_text.size();
    put(&l_text, 4);
    put(header_text.data(), header_text.size());
    const int32_t n_ref = (int32_t)ref_names.size();
    put(&n_ref, 4);
    for (int32_t i = 0; i < n_ref; ++i) {
        const int32_t l_name = (int32_t)ref_names[i].size() + 1;
        put(&l_name, 4);
        put(ref_names[i].c_str(), (size_t)l_name);
        put(&ref_len[i], 4);
    }
}

static int reg2bin(int64_t beg, int64_t end) {  // SAM spec 5.3
    --end;
    if (beg >> 14 == end >> 14) return (int)(((1 << 15) - 1) / 7 + (beg >> 14));
    if (beg >> 17 == end >> 17) return (int)(((1 << 12) - 1) / 7 + (beg >> 17));
    if (beg >> 20 == end >> 20) return (int)(((1 << 9) - 1) / 7 + (beg >> 20));
    if (beg >> 23 == end >> 23) return (int)(((1 << 6) - 1) / 7 + (beg >> 23));
    if (beg >> 26 == end >> 26) return (int)(((1 << 3) - 1) / 7 + (beg >> 26));
    return 0;
}

void BamWriter::write_record(const std::string &line) {
    std::vector<uint8_t> r;
    encode_record(line, r);
    put(r.data(), r.size());
}

// (r04: no allocation per record or field -- fields are (pointer, length) views of the line, the record is built in
// place behind dst, bases go through a 256-entry table; 8 M records: 0.66 -> 0.2 s of SAM -> BAM on 16 threads)
namespace {
struct Field {
    const char *p;
    size_t n;
    bool is(const char *lit) const { return n == strlen(lit) && memcmp(p, lit, n) == 0; }
};
// strtol / strtoul / strtoll on a field that is not NUL-terminated: optional blanks and sign, digits up to the first other byte
long long field_int(const char *p, size_t n) {
    size_t i = 0;
    while (i < n && (p[i] == ' ' || p[i] == '\t')) ++i;
    bool neg = false;
    if (i < n && (p[i] == '+' || p[i] == '-')) neg = p[i++] == '-';
    unsigned long long v = 0;
    for (; i < n && p[i] >= '0' && p[i] <= '9'; ++i) v = v * 10 + (unsigned)(p[i] - '0');
    return neg ? -(long long)v : (long long)v;
}
float field_float(const char *p, size_t n) {
    char tmp[64];
    const size_t k = n < sizeof(tmp) - 1 ? n : sizeof(tmp) - 1;
    memcpy(tmp, p, k);
    tmp[k] = 0;
    return strtof(tmp, nullptr);
}
struct NibbleTable {  // base (either case) -> its code in kBamSeq, 15 ('N') for anything else
    uint8_t code[256];
    NibbleTable() {
        memset(code, 15, sizeof(code));
        for (int k = 0; k < 16; ++k) {
            code[(uint8_t)kBamSeq[k]] = (uint8_t)k;
            if (kBamSeq[k] >= 'A' && kBamSeq[k] <= 'Z') code[(uint8_t)(kBamSeq[k] + 32)] = (uint8_t)k;
        }
    }
};
const NibbleTable kNibble;
template <class T>
void put_le(std::vector<uint8_t> &r, T v) {
    r.insert(r.end(), (const uint8_t *)&v, (const uint8_t *)&v + sizeof(T));
}
}  // namespace

void BamWriter::encode_record(const std::string &line, std::vector<uint8_t> &dst) const {
    Field fld[11];
    // optional fields: the first 32 in place (every tagged record has at least one: a local vector allocated per record),
    // a vector only for a record with more
    Field opt[32];
    std::vector<Field> opt_more;
    size_t n_opt = 0;
    size_t nf = 0;
    {
        const char *d = line.data();
        const size_t n = line.size();
        size_t b = 0;
        for (;;) {
            const void *t = b <= n ? memchr(d + b, '\t', n - b) : nullptr;
            const size_t e = t ? (size_t)((const char *)t - d) : n;
            if (nf < 11) fld[nf] = Field{d + b, e - b};
            else if (n_opt < 32) opt[n_opt++] = Field{d + b, e - b};
            else opt_more.push_back(Field{d + b, e - b}), ++n_opt;
            ++nf;
            if (!t) break;
            b = e + 1;
        }
    }
    if (nf < 11) bail("Error writing record to output file: too few SAM fields");
    if (fld[0].n > 254) bail("Error writing record to output file: read name longer than 254 bytes");  // l_read_name is one byte
    auto ref_id = [&](const Field &f) -> int32_t {
        if (f.is("*")) return -1;
        for (size_t i = 0; i < ref_names.size(); ++i)
            if (ref_names[i].size() == f.n && memcmp(ref_names[i].data(), f.p, f.n) == 0) return (int32_t)i;
        return -1;
    };
    const size_t start = dst.size();
    std::vector<uint8_t> &r = dst;  // built in place: block_size is patched in at the end
    put_le<int32_t>(r, 0);
    const int32_t rid = ref_id(fld[2]), pos = (int32_t)field_int(fld[3].p, fld[3].n) - 1;
    const uint8_t mapq = (uint8_t)field_int(fld[4].p, fld[4].n);
    const uint16_t flag = (uint16_t)field_int(fld[1].p, fld[1].n);
    uint32_t cig[64];
    std::vector<uint32_t> cig_more;
    size_t n_cig_ops = 0;
    int64_t ref_span = 0;
    if (!fld[5].is("*")) {
        const char *c = fld[5].p, *const ce = c + fld[5].n;
        while (c < ce) {
            uint32_t len = 0;
            while (c < ce && *c >= '0' && *c <= '9') len = len * 10 + (uint32_t)(*c++ - '0');
            static const char ops[] = "MIDNSHP=X";
            const char *o = c < ce ? (const char *)memchr(ops, *c, 9) : nullptr;
            if (!o) bail("Error writing record to output file: bad CIGAR");
            const uint32_t op = (uint32_t)(o - ops);
            if (n_cig_ops < 64) cig[n_cig_ops] = len << 4 | op;
            else cig_more.push_back(len << 4 | op);
            ++n_cig_ops;
            if (op == 0 || op == 2 || op == 3 || op == 7 || op == 8) ref_span += len;
            ++c;
        }
    }
    const Field &seq = fld[9];
    const int32_t l_seq = seq.is("*") ? 0 : (int32_t)seq.n;
    const int32_t next_rid = fld[6].is("=") ? rid : ref_id(fld[6]);
    const int32_t next_pos = (int32_t)field_int(fld[7].p, fld[7].n) - 1, tlen = (int32_t)field_int(fld[8].p, fld[8].n);
    const uint8_t l_name = (uint8_t)(fld[0].n + 1);
    const uint16_t bin = (uint16_t)reg2bin(pos, pos + (ref_span ? ref_span : 1)), n_cig = (uint16_t)n_cig_ops;
    put_le(r, rid), put_le(r, pos), put_le(r, l_name), put_le(r, mapq), put_le(r, bin), put_le(r, n_cig), put_le(r, flag);
    put_le(r, l_seq), put_le(r, next_rid), put_le(r, next_pos), put_le(r, tlen);
    r.insert(r.end(), (const uint8_t *)fld[0].p, (const uint8_t *)fld[0].p + (l_name - 1));
    r.push_back(0);
    for (size_t k = 0; k < n_cig_ops; ++k) put_le<uint32_t>(r, k < 64 ? cig[k] : cig_more[k - 64]);
    {
        const size_t at = r.size();
        r.resize(at + (size_t)(l_seq + 1) / 2 + (size_t)l_seq);
        uint8_t *o = r.data() + at;
        const uint8_t *sq = (const uint8_t *)seq.p;
        int32_t k = 0;
        for (; k + 1 < l_seq; k += 2) *o++ = (uint8_t)(kNibble.code[sq[k]] << 4 | kNibble.code[sq[k + 1]]);
        if (k < l_seq) *o++ = (uint8_t)(kNibble.code[sq[k]] << 4);
        if (fld[10].is("*")) {
            memset(o, 0xFF, (size_t)l_seq);
        } else {
            if ((int32_t)fld[10].n != l_seq) bail("Error writing record to output file: SEQ and QUAL lengths differ");
            const uint8_t *q = (const uint8_t *)fld[10].p;
            for (int32_t i = 0; i < l_seq; ++i) o[i] = (uint8_t)(q[i] - 33);
        }
    }
    for (size_t ti = 0; ti < n_opt; ++ti) {  // TAG:TYPE:VALUE
        const Field &t = ti < 32 ? opt[ti] : opt_more[ti - 32];
        if (t.n < 5 || t.p[2] != ':' || t.p[4] != ':') bail("Error writing record to output file: bad optional field");
        r.insert(r.end(), (const uint8_t *)t.p, (const uint8_t *)t.p + 2);
        const char type = t.p[3];
        const char *v = t.p + 5;
        const size_t vn = t.n - 5;
        if (type == 'A') {
            r.push_back('A');
            r.push_back(vn == 0 ? 0 : (uint8_t)v[0]);
        } else if (type == 'i') {  // smallest integer type that holds the value, like samtools
            const long long x = field_int(v, vn);
            if (x >= 0) {
                if (x <= 0xff) r.push_back('C'), put_le(r, (uint8_t)x);
                else if (x <= 0xffff) r.push_back('S'), put_le(r, (uint16_t)x);
                else r.push_back('I'), put_le(r, (uint32_t)x);
            } else {
                if (x >= -128) r.push_back('c'), put_le(r, (int8_t)x);
                else if (x >= -32768) r.push_back('s'), put_le(r, (int16_t)x);
                else r.push_back('i'), put_le(r, (int32_t)x);
            }
        } else if (type == 'f') {
            r.push_back('f');
            put_le(r, field_float(v, vn));
        } else if (type == 'Z' || type == 'H') {
            r.push_back((uint8_t)type);
            r.insert(r.end(), (const uint8_t *)v, (const uint8_t *)v + vn);
            r.push_back(0);
        } else if (type == 'B') {
            r.push_back('B');
            const char sub = vn == 0 ? 'c' : v[0];
            r.push_back((uint8_t)sub);
            const size_t cnt_at = r.size();
            put_le<int32_t>(r, 0);
            int32_t cnt = 0;
            size_t q = 1;
            while (q < vn) {  // ",a,b,c"
                const void *c = memchr(v + q + 1, ',', vn - q - 1);
                const size_t e = c ? (size_t)((const char *)c - v) : vn;
                const char *it = v + q + 1;
                const size_t in = e - q - 1;
                switch (sub) {
                case 'c': put_le(r, (int8_t)field_int(it, in)); break;
                case 'C': put_le(r, (uint8_t)field_int(it, in)); break;
                case 's': put_le(r, (int16_t)field_int(it, in)); break;
                case 'S': put_le(r, (uint16_t)field_int(it, in)); break;
                case 'i': put_le(r, (int32_t)field_int(it, in)); break;
                case 'I': put_le(r, (uint32_t)field_int(it, in)); break;
                case 'f': put_le(r, field_float(it, in)); break;
                default: bail("Error writing record to output file: bad B array subtype");
                }
                ++cnt;
                if (!c) break;
                q = e;
            }
            memcpy(r.data() + cnt_at, &cnt, 4);
        } else {
            bail("Error writing record to output file: unknown optional field type");
        }
    }
    const int32_t block_size = (int32_t)(r.size() - start - 4);
    memcpy(r.data() + start, &block_size, 4);
}

void BamWriter::close() {
    if (!f) return;
    std::exception_ptr err;
    try {
        flush(true);
    } catch (...) {
        err = std::current_exception();
    }
    {
        std::lock_guard<std::mutex> lk(mu_);
        closing_ = true;
    }
    cv_.notify_all();
    if (writer_.joinable()) writer_.join();
    if (!err && failed_) err = failed_;
    static const uint8_t eof[28] = {0x1f, 0x8b, 8, 4, 0, 0, 0, 0, 0, 0xff, 6, 0, 'B', 'C', 2, 0, 0x1b, 0, 3, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    if (!err) fwrite(eof, 1, sizeof(eof), f);
    fclose(f);
    f = nullptr;
    if (codec_) mk_codec_destroy((mk_codec *)codec_), codec_ = nullptr;
    for (HostBuffer &b : free_raw_) b.reset();  // (freed at close, not kept to the end of the process)
    free_raw_.clear();
    closing_ = false;
    failed_ = nullptr;
    if (err) std::rethrow_exception(err);
}

void BamWriter::append_tagged_raw(const uint8_t *rec, uint32_t len, const std::string &tag, const char *val, size_t val_len,
                                  std::vector<uint8_t> &dst) {
    const int32_t block_size = (int32_t)(len + 3 + val_len + 1);
    dst.insert(dst.end(), (const uint8_t *)&block_size, (const uint8_t *)&block_size + 4);
    dst.insert(dst.end(), rec, rec + len);
    dst.push_back((uint8_t)tag[0]);
    dst.push_back((uint8_t)tag[1]);
    dst.push_back('Z');
    dst.insert(dst.end(), (const uint8_t *)val, (const uint8_t *)val + val_len);
    dst.push_back(0);
}

}  // namespace cli
