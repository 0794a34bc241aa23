#include "chunk_reader.hpp"

#include <cstring>

#include "../../../include/lash_gfx950.h"

namespace lashhost {

int sniff_format(const uint8_t *p, uint64_t n)
{
    if (n == 0) return 0;
    return p[0] == '>' ? LASH_FMT_FASTA : p[0] == '@' ? LASH_FMT_FASTQ : 0;
}

std::string error_not_fastx(const std::string &path) { return "Invalid input file: neither FASTA ('>') nor FASTQ ('@'): " + path; }

std::string error_not_fasta(const std::string &flag, const std::string &path)
{
    return flag + " takes FASTA input; this file starts with '@' (FASTQ): " + path;
}

// FASTA: before the last '\n>' of the second half when there is one (nothing to carry).  Otherwise the record continues
// in the next chunk: cut at the last line end (or at the chunk end inside one enormous line) and carry the last <= 32
// SURVIVING bases of the current record as a synthetic sequence line.  Those are exactly the bases a k-mer spanning the
// cut can reach back to (k - 1 <= 31; filter_out_n deletes everything else anyway), so the k-mer set of the pieces
// equals that of the whole record however long an N run at the cut is; the few k-mers inside the carried line are
// repeats, which max / OR ignore.  FASTQ: before the last complete record start of the second half; nothing carried.
size_t find_cut(const uint8_t *b, size_t n, int fmt, std::vector<uint8_t> &carry)
{
    carry.clear();
    if (fmt == LASH_FMT_FASTA) {
        for (size_t q = n - 1; q > n / 2; --q)
            if (b[q] == '>' && b[q - 1] == '\n') return q;
        size_t cut = n;
        while (cut > n / 2 && b[cut - 1] != '\n') --cut;
        if (cut <= n / 2) cut = n;                        // one enormous line: cut inside it
        // walk back line by line from the cut, collecting surviving bases, until 32 are found or a header line is met
        std::vector<uint8_t> rev;                         // collected bases, last one first
        size_t line_stop = cut;                           // one past the last byte of the line being looked at
        while (rev.size() < 32 && line_stop > 0) {
            size_t ls = line_stop;                        // start of that line
            if (ls > 0 && b[ls - 1] == '\n') --ls;        // (step over the terminator of the previous line)
            while (ls > 0 && b[ls - 1] != '\n') --ls;
            if (b[ls] == '>') break;                      // the record began here: nothing before it belongs to it
            for (size_t i = line_stop; i > ls && rev.size() < 32; --i) {
                const uint8_t ch = b[i - 1];
                if (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T') rev.push_back(ch);
            }
            line_stop = ls;
        }
        if (!rev.empty()) {
            carry.assign(rev.rbegin(), rev.rend());
            carry.push_back('\n');
        }
        return cut;
    }
    auto line_end = [&](size_t p) { const void *e = memchr(b + p, '\n', n - p); return e ? (size_t)((const uint8_t *)e - b) : n; };
    for (size_t q = n - 1; q > n / 2; --q) {
        if (b[q] != '@' || b[q - 1] != '\n') continue;
        const size_t e1 = line_end(q);
        if (e1 >= n) continue;
        const size_t e2 = line_end(e1 + 1);
        if (e2 >= n || e2 + 1 >= n) continue;
        if (b[e2 + 1] == '+') return q;
    }
    return 0;                                             // no FASTQ record boundary in the second half
}

std::string ChunkReader::fill(uint8_t *b, size_t have)
{
    std::string err;
    while (have < chunk_) {
        const long r = bs_.read(b + have, chunk_ - have, err);
        if (r < 0) return err + " (" + path_ + ")";
        if (r == 0) { eof_ = true; break; }
        have += (size_t)r;
        total_ += (uint64_t)r;
    }
    have_ = have;
    return "";
}

std::string ChunkReader::classify(const uint8_t *b)
{
    if (classified_) return "";
    classified_ = true;
    if (have_ == 0) return "Invalid input file: empty (" + path_ + ")";
    fmt_ = sniff_format(b, have_);
    if (!fmt_) return error_not_fastx(path_);
    if (rule_ == CutRule::whole_records && fmt_ != LASH_FMT_FASTA) return error_not_fasta(rule_text_, path_);
    return "";
}

std::string ChunkReader::cut(const uint8_t *b)
{
    carry_.clear();
    cut_ = have_;
    if (eof_ || rule_ == CutRule::none) return "";
    if (rule_ == CutRule::whole_records) {
        for (cut_ = have_ - 1; cut_ > 0 && !(b[cut_] == '>' && b[cut_ - 1] == '\n'); --cut_) {}
        if (cut_) return "";
        size_t id_end = 1;
        while (id_end < have_ && id_end < 200 && b[id_end] != ' ' && b[id_end] != '\t' && b[id_end] != '\r' && b[id_end] != '\n') ++id_end;
        return "record '" + std::string(reinterpret_cast<const char *>(b) + 1, id_end - 1) + "' of " + path_ + " does not fit in a chunk of " +
               std::to_string(chunk_ >> 20) + " MiB: " + rule_text_ + " never splits a record, raise --stream-mb";
    }
    cut_ = find_cut(b, have_, fmt_, carry_);
    if (rule_ == CutRule::between_records && !carry_.empty()) return rule_text_;
    if (cut_ == 0) return "cannot find a record boundary inside a " + std::to_string(chunk_ >> 20) + " MiB chunk of " + path_;
    return "";
}

size_t ChunkReader::move_rest(const uint8_t *b, uint8_t *dst) const
{
    if (have_ > cut_) memmove(dst + carry_.size(), b + cut_, have_ - cut_);      // first: dst may be b
    if (!carry_.empty()) memcpy(dst, carry_.data(), carry_.size());
    return rest();
}

}  // namespace lashhost
