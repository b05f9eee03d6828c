// bam_text.hpp -- BAM records as SAM text: the nibble alphabet, a bounded cursor over a record's bytes, and the line of a record
#pragma once
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "util.hpp"

namespace cli {

// the base of every 4-bit code of a packed BAM sequence (SAM spec 4.2.3)
inline constexpr char kBamSeq[] = "=ACMGRSVTWYHKDBN";

// the bytes [p, e) of a BAM record, taken in order; reading past e is the truncated-file error
struct Cur {
    const uint8_t *p, *e;
    template <class T>
    T get() {
        if ((size_t)(e - p) < sizeof(T)) bail("Error during BAM record parsing: truncated file");
        T v;
        memcpy(&v, p, sizeof(T));
        p += sizeof(T);
        return v;
    }
    const uint8_t *take(size_t n) {
        if ((size_t)(e - p) < n) bail("Error during BAM record parsing: truncated file");
        const uint8_t *r = p;
        p += n;
        return r;
    }
};

// the optional fields from c.p to c.e as SAM text, each with a TAB in front, appended to out
void aux_to_text(Cur &c, std::string &out);
// one BAM alignment record (at its block_size field) -> SAM text line appended to s
void bam_record_to_sam(const uint8_t *at, const std::vector<std::string> &refs, std::string &s);

}  // namespace cli
