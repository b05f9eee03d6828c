// test harness: the host loop of `merkurio tag` (merkurio_amd/csrc/cli/tag_host.cpp: TagHostLoop::run) WITHOUT a device, over the whole
// input in one go or as <turns> bounded turns one after the other, the way cli/tag_windows.cpp gives the loop the windows the device
// refused: SAM text cut at line starts (SamFile::seek_text with an end), BAM cut at BGZF members with the record that crosses a
// cut carried over as the next turn's head (SamFile::seek_bam with an end member, SamFile::bam_pending).  The matcher is a stub that
// keeps every record and finds nothing, so the tag value is the record's existing one or empty.  Output: SAM text or BAM (zlib on the
// host threads) by the output's extension.
// usage: harness <in.sam|in.bam> <out.sam|out.bam> <turns: 0 = the whole file> <window MiB of the loop's reads>
// prints "#turn <k> head <bytes carried into turn k>" per turn and "#records <n>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

#include "tag_host.hpp"
using namespace cli;

extern "C" {
int mk_tag_records(mk_matcher *, const uint8_t *, const uint64_t *off, uint64_t n_rec, int, int, int, uint8_t *keep, mk_row *, uint64_t, uint64_t *n_rows,
                   mk_counters *counters, uint32_t *, uint64_t *found_off, uint32_t *, uint64_t) {
    memset(keep, 1, n_rec);
    *n_rows = 0;
    for (uint64_t i = 0; i <= n_rec; ++i) found_off[i] = 0;
    counters->nb_records_tot += n_rec, counters->nb_bases += off[n_rec], counters->nb_records_extracted += n_rec;
    return MK_OK;
}
int mk_tag_value(const mk_matcher *, const uint32_t *, uint64_t, const char *existing, char *out, size_t cap, size_t *out_len) {
    *out_len = existing ? strlen(existing) : 0;
    if (*out_len + 1 > cap) return MK_E_CAPACITY;
    memcpy(out, existing ? existing : "", *out_len + 1);
    return MK_OK;
}
const char *mk_last_error(void) { return "stub"; }
}

int main(int argc, char **argv) {
    if (argc != 5) return 2;
    try {
        TagArgs a;
        a.in_file = argv[1];
        a.window_mb = atoi(argv[4]);
        const std::string out = argv[2];
        const size_t turns = (size_t)atoi(argv[3]);
        const bool to_bam = out.size() > 4 && out.substr(out.size() - 4) == ".bam";
        SamFile sam;
        sam.open(a.in_file);
        Sink w;
        BamWriter bw;
        if (to_bam) {
            if (sam.is_bam) bw.open(out, sam.header, &sam.ref_names, &sam.ref_lens);
            else bw.open(out, sam.header);
        } else {
            w.open(out);
            w.write(sam.header);
        }
        Loggers lg;
        Patterns pats;
        PhaseTimer tm;
        tm.on = false;
        mk_counters c;
        memset(&c, 0, sizeof(c));
        std::vector<uint32_t> counts;
        const TagHandle h{nullptr, 0, &c, &counts};
        TagHostLoop host(a, sam, lg, pats, "in", w, bw, to_bam, tm, {h});
        if (turns == 0) {
            host.run();
        } else if (!sam.is_bam) {
            const char *text = sam.source().text();
            const uint64_t n = sam.source().text_size(), b0 = sam.text_cursor();
            uint64_t b = b0;
            for (size_t k = 0; k < turns; ++k) {
                uint64_t e = k + 1 == turns ? n : std::max(b, b0 + (n - b0) * (k + 1) / turns);
                while (e < n && e > b && text[e - 1] != '\n') ++e;
                printf("#turn %zu head 0\n", k);
                sam.seek_text(b, e);
                host.run(&h);
                b = e;
            }
        } else {
            uint64_t n_head = 0;
            const char *p = sam.bam_pending(&n_head);
            std::string head(p, n_head);
            const size_t m0 = sam.source().next_member(), n_mem = sam.source().n_bgzf_members();
            size_t m = m0;
            for (size_t k = 0; k < turns; ++k) {
                const size_t m1 = k + 1 == turns ? n_mem : m0 + (n_mem - m0) * (k + 1) / turns;
                printf("#turn %zu head %zu\n", k, head.size());
                sam.seek_bam(m, head.data(), head.size(), m1);
                host.run(&h);
                p = sam.bam_pending(&n_head);
                head.assign(p, n_head);
                m = m1;
            }
        }
        w.flush();
        bw.close();
        printf("#records %llu\n", (unsigned long long)c.nb_records_tot);
    } catch (const Error &e) {
        printf("#error %s\n", e.what());
    }
    return 0;
}
