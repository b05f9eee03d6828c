#include "bam_text.hpp"

namespace cli {

void aux_to_text(Cur &c, std::string &out) {
    while (c.p < c.e) {
        const uint8_t *tag = c.take(2);
        char type = (char)c.get<uint8_t>();
        out += '\t';
        out.append((const char *)tag, 2);
        char buf[64];
        switch (type) {
        case 'A': out += ":A:"; out += (char)c.get<uint8_t>(); break;
        case 'c': out += ":i:" + std::to_string((int)c.get<int8_t>()); break;
        case 'C': out += ":i:" + std::to_string((unsigned)c.get<uint8_t>()); break;
        case 's': out += ":i:" + std::to_string((int)c.get<int16_t>()); break;
        case 'S': out += ":i:" + std::to_string((unsigned)c.get<uint16_t>()); break;
        case 'i': out += ":i:" + std::to_string(c.get<int32_t>()); break;
        case 'I': out += ":i:" + std::to_string(c.get<uint32_t>()); break;
        case 'f': snprintf(buf, sizeof(buf), "%g", (double)c.get<float>()); out += ":f:"; out += buf; break;
        case 'Z':
        case 'H': {
            out += type == 'Z' ? ":Z:" : ":H:";
            const uint8_t *s = c.p;
            while (c.p < c.e && *c.p) ++c.p;
            out.append((const char *)s, c.p - s);
            if (c.p < c.e) ++c.p;
            break;
        }
        case 'B': {
            char sub = (char)c.get<uint8_t>();
            int32_t cnt = c.get<int32_t>();
            out += ":B:";
            out += sub;
            for (int32_t k = 0; k < cnt; ++k) {
                out += ',';
                switch (sub) {
                case 'c': out += std::to_string((int)c.get<int8_t>()); break;
                case 'C': out += std::to_string((unsigned)c.get<uint8_t>()); break;
                case 's': out += std::to_string((int)c.get<int16_t>()); break;
                case 'S': out += std::to_string((unsigned)c.get<uint16_t>()); break;
                case 'i': out += std::to_string(c.get<int32_t>()); break;
                case 'I': out += std::to_string(c.get<uint32_t>()); break;
                case 'f': snprintf(buf, sizeof(buf), "%g", (double)c.get<float>()); out += buf; break;
                default: bail("Error during BAM record parsing: bad B array subtype");
                }
            }
            break;
        }
        default: bail("Error during BAM record parsing: unknown tag type");
        }
    }
}

void bam_record_to_sam(const uint8_t *at, const std::vector<std::string> &refs, std::string &s) {
    static const char kCig[] = "MIDNSHP=X";
    const int32_t n_ref = (int32_t)refs.size();
    int32_t block;
    memcpy(&block, at, 4);
    Cur r{at + 4, at + 4 + block};
    int32_t ref_id = r.get<int32_t>(), pos = r.get<int32_t>();
    uint8_t l_name = r.get<uint8_t>(), mapq = r.get<uint8_t>();
    (void)r.get<uint16_t>();
    uint16_t n_cig = r.get<uint16_t>(), flag = r.get<uint16_t>();
    int32_t l_seq = r.get<int32_t>(), next_ref = r.get<int32_t>(), next_pos = r.get<int32_t>(), tlen = r.get<int32_t>();
    const uint8_t *nm = r.take(l_name);
    s.reserve(s.size() + (size_t)block + (size_t)l_seq + 64);
    s.append((const char *)nm, l_name ? l_name - 1u : 0u);
    s += '\t' + std::to_string(flag) + '\t';
    s += ref_id >= 0 && ref_id < n_ref ? refs[ref_id] : "*";
    s += '\t' + std::to_string(pos + 1) + '\t' + std::to_string(mapq) + '\t';
    if (n_cig == 0) s += '*';
    for (uint16_t k = 0; k < n_cig; ++k) {
        uint32_t v = r.get<uint32_t>();
        s += std::to_string(v >> 4);
        s += (v & 15) < 9 ? kCig[v & 15] : '?';
    }
    s += '\t';
    s += next_ref < 0 ? "*" : (next_ref == ref_id ? "=" : (next_ref < n_ref ? refs[next_ref] : "*"));
    s += '\t' + std::to_string(next_pos + 1) + '\t' + std::to_string(tlen) + '\t';
    if (l_seq < 0) bail("Error during BAM record parsing: truncated file");
    const uint8_t *sq = r.take(((size_t)l_seq + 1) / 2);
    if (l_seq == 0) {
        s += '*';
    } else {
        const size_t at0 = s.size();
        s.resize(at0 + (size_t)l_seq);
        for (int32_t k = 0; k < l_seq; ++k) s[at0 + k] = kBamSeq[(sq[k >> 1] >> ((~k & 1) << 2)) & 15];
    }
    s += '\t';
    const uint8_t *ql = r.take((size_t)l_seq);
    if (l_seq == 0 || ql[0] == 0xFF) {
        s += '*';
    } else {
        const size_t at0 = s.size();
        s.resize(at0 + (size_t)l_seq);
        for (int32_t k = 0; k < l_seq; ++k) s[at0 + k] = (char)(ql[k] + 33);
    }
    aux_to_text(r, s);
}

}  // namespace cli
