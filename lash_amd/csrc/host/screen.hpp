// screen.hpp — `lash screen` (not upstream; Mash's `screen -w`): what is in a sample.  Every reference of a database is scored against a
// sample by the containment of the reference in it, and a shared k-mer is credited only to the best reference that holds it (winner
// takes all): the thousands of near-identical references one genome of the sample lights up fall away, each re-scored on what it has
// left.  HyperMinHash collections, resolved on the GPU (lash_sketch_set_screen_wta).
#pragma once
#include <string>

#include "dist.hpp"

namespace lashhost {

struct ScreenOptions {
    DistOptions side;          // ref_prefix (-r, the database), query_prefix (-q, the samples), model, threads, file_order, block_rows, device, layout
    std::string output;        // -o FILE: the table
    bool has_max_dist = false; // --max-dist D: candidates and printed rows pass d <= D; without it D = nextafter(1, 0): a positive similarity
    double max_dist = 0.0;
    bool keep_losers = false;  // --keep-losers: also the candidates whose winner-takes-all distance no longer passes
};

// "" or why D is refused: a number in [0, 1]
std::string check_screen_max_dist(double d);

std::string run_screen(const ScreenOptions &opt);

}  // namespace lashhost
