// cli_args.hpp — the argument layer of the `lash` commands (main.cpp): one option table per command, typed getters that print
// the refusal themselves, and the checks several commands share.  A getter leaves its output alone when the option was not
// given and returns false after printing "error: ..."; the caller then returns exit code 2.
#pragma once
#include <cstdint>
#include <initializer_list>
#include <map>
#include <string>
#include <vector>

#include "dist.hpp"

namespace lashhost {

struct Option {
    const char *name;       // --name
    char letter;            // -x, or 0
    bool takes_value;       // false: a flag
};

// The options of one command; every command has --help besides.  A closed set refuses any other --name, wherever it stands.
struct Command {
    std::vector<Option> options;
    bool closed;
};

// One row of an option's exclusions.  {"dm", "why"} hits when --dm was given: "--A cannot be used with --dm (why)".
// {nullptr, text, hit} hits when `hit` is true: "--A text".
struct Rule {
    const char *other;
    std::string text;
    bool hit = false;
};

class Args {
public:
    bool parse(int argc, char **argv, const Command &cmd);
    bool has(const char *name) const { return kv.count(name) || flags.count(name); }
    std::string str(const char *name, const char *otherwise = "") const { return kv.count(name) ? kv.at(name) : otherwise; }

    bool invalid(const char *name) const;                                 // "invalid value for --name"
    bool invalid(const char *name, const std::string &required) const;    // "invalid value 'V' for --name: required"
    // an unsigned integer; the second form also holds it within [lo, hi] and answers in the quoted form
    bool u64(const char *name, uint64_t &v) const;
    bool u64(const char *name, uint64_t &v, uint64_t lo, uint64_t hi, const std::string &required) const;
    // a number that strtod reads to the end and `ok` accepts (default: any finite one)
    bool real(const char *name, double &v, bool (*ok)(double) = nullptr, const std::string &required = "a finite number is required") const;
    // the place of the value in `words`; with required == nullptr nothing is printed
    bool choice(const char *name, std::initializer_list<const char *> words, int &index, const char *required) const;
    // a comma list of integers in [lo, hi]; false, in silence, at the first item that is not one (out holds the items before it)
    bool u64_list(const char *name, std::vector<uint64_t> &out, uint64_t lo = 0, uint64_t hi = UINT64_MAX) const;
    // {name, placeholder} rows; all_lines: name every row when any is missing (dist), otherwise only the missing ones
    bool require(std::initializer_list<std::pair<const char *, const char *>> rows, bool all_lines = false) const;
    // the exclusions of --name, when it was given: the first rule that hits is printed
    bool allowed(const char *name, std::initializer_list<Rule> rules) const;

private:
    std::map<std::string, std::string> kv;
    std::map<std::string, bool> flags;
};

// --devices D[,D...] (sketch, dist): appended to `devices`
bool devices_option(const Args &a, std::vector<int> &devices);
// --hll-bias FILE / --hll-bias-sim / $LASH_HLL_BIAS (dist, growth)
bool bias_source(const Args &a, DistOptions &side);
// -t (at least 1; default: all logical cores), --device, --file-order
bool threads_device_order(const Args &a, DistOptions &side);
// --layout / $LASH_LAYOUT
bool layout_option(const Args &a, lash_layout &layout);
// --groups FILE | --all NAME (merge: one of them is required; spectrum: neither means --all all)
bool groups_or_all(const Args &a, bool required, std::string &groups_file, std::string &all_name);
// the end of a command: "Error: ..." and 1, or the closing line on stdout and 0
int finish(const std::string &err, const char *done);

}  // namespace lashhost
