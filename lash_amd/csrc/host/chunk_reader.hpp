// chunk_reader.hpp — a file above --stream-mb, read in chunks that end where the route's cut rule allows (sketch_files.cpp: the plain
// streamed route, --min-count / --aa, --per-record / --window).  One step per method; the buffers are the caller's:
//     while (!rd.eof()) { rd.fill(b, have); rd.classify(b); rd.cut(b); ...use b[0, rd.cut_at())...; have = rd.move_rest(b, next); }
#pragma once
#include <cstddef>
#include <cstdint>
#include <string>
#include <vector>

#include "fastx.hpp"

namespace lashhost {

enum class CutRule {
    none,             // no cut: the caller only wants the bytes (or their count)
    carry,            // find_cut: FASTA may be cut inside a record, the next chunk then starts with a carried line of <= 32 bases; FASTQ is
                      // cut before a record start of the second half
    between_records,  // find_cut, but a record that spans the cut is the caller's error (`rule_text`)
    whole_records     // FASTA only: before the last '>' that follows a '\n', anywhere after the chunk's first byte
};

// '>' => LASH_FMT_FASTA, '@' => LASH_FMT_FASTQ, anything else (or no byte at all) => 0: needletail decides by the first byte of the
// (decompressed) file and fails on anything else (parse_fastx_file, utils.rs:453)
int sniff_format(const uint8_t *p, uint64_t n);
std::string error_not_fastx(const std::string &path);                            // "Invalid input file: neither FASTA ..."
std::string error_not_fasta(const std::string &flag, const std::string &path);   // "<flag> takes FASTA input ..."

// Where to end this chunk of a file that is streamed in pieces (0 = no boundary found), and what the next chunk has to start with.
size_t find_cut(const uint8_t *b, size_t n, int fmt, std::vector<uint8_t> &carry);

class ChunkReader {
public:
    // rule_text — between_records: the error text for a record longer than a chunk; whole_records: the option that asked ("--per-record")
    ChunkReader(const std::string &path, size_t chunk_bytes, int threads, CutRule rule, const std::string &rule_text = "")
        : path_(path), chunk_(chunk_bytes), rule_(rule), rule_text_(rule_text) { bs_.set_threads(threads); }
    // every step returns "" or the error text
    std::string open() { return bs_.open(path_); }
    std::string fill(uint8_t *b, size_t have);       // b[0, have) is there already; reads on up to the chunk size or the end of the file
    std::string classify(const uint8_t *b);          // the first chunk decides the format (later calls return "")
    std::string cut(const uint8_t *b);               // the chunk ends at cut_at(); all of it at the end of the file
    // what the next chunk starts with — the carried line, then the bytes after the cut — to dst (which may be b); returns their count
    size_t move_rest(const uint8_t *b, uint8_t *dst) const;

    bool eof() const { return eof_; }
    int fmt() const { return fmt_; }
    size_t cut_at() const { return cut_; }
    size_t rest() const { return carry_.size() + (have_ - cut_); }
    const std::vector<uint8_t> &carry() const { return carry_; }
    uint64_t bytes_read() const { return total_; }   // of the uncompressed file, so far

private:
    ByteStream bs_;
    std::string path_;
    size_t chunk_;
    CutRule rule_;
    std::string rule_text_;
    std::vector<uint8_t> carry_;
    size_t have_ = 0, cut_ = 0;
    uint64_t total_ = 0;
    int fmt_ = 0;
    bool eof_ = false, classified_ = false;
};

}  // namespace lashhost
