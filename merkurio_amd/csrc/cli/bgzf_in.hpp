// bgzf_in.hpp -- BGZF input (BAM, bgzip'ed FASTA/FASTQ): the member table of a file, runs of members, and their inflate on the
// device codec or on the host threads.  One member is the ABI's mk_bgzf_member everywhere.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../../include/merkurio_hip.h"

namespace cli {

// BGZF = a series of gzip members, each with the extra subfield 'B','C' holding the member's size (SAM spec 4.1).  The member table
// of d[0, n): data_off absolute in the file, out_off the running text offset.  false if the file is not BGZF all the way through
// (FLG exactly FEXTRA, whole members to the last byte): the caller falls back to the serial gzip reader.
bool bgzf_walk(const uint8_t *d, size_t n, std::vector<mk_bgzf_member> &mem);
// A run of members worth about want_text bytes of text: the first member behind m0 that is not taken.  At least one member is taken,
// then more while the text so far is less than want_text; never past min(m.size(), m_end).
size_t bgzf_run_end(const std::vector<mk_bgzf_member> &m, size_t m0, size_t m_end, uint64_t want_text);
// the run m[0, n) for a window that starts at byte file_lo of the file and at byte text_base of the text
std::vector<mk_bgzf_member> bgzf_rebased(const mk_bgzf_member *m, size_t n, uint64_t file_lo, uint64_t text_base);

// BGZF input is inflated by the device codec on this HIP device from now on (windows of at least a few hundred members; < 0: zlib
// on the host threads); seconds spent in those calls so far
void set_bgzf_device(int device, bool always = false);
double bgzf_device_seconds();
// inflates mem[0, cnt) of the file d into out + (member.out_off - mem[0].out_off): on the device where set_bgzf_device() chose one and
// the caller allows it (one lane per member, mk_bgzf_inflate: stream errors, ISIZE and CRC-32 checked there), else on the host threads
void bgzf_inflate_range(const uint8_t *d, const mk_bgzf_member *mem, size_t cnt, char *out, const std::string &path, bool may_use_device = true);
// BGZF members inflated by zlib on the host threads, whatever set_bgzf_device() says: out + member.out_off receives each
// member's text (the host checker of windows the device refused or could not hold); CRC-32 and ISIZE checked
void inflate_bgzf_members_host(const uint8_t *file, const mk_bgzf_member *members, size_t n, char *out, const std::string &path);

}  // namespace cli
