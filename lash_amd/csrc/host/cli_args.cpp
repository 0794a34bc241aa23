// cli_args.cpp — see cli_args.hpp
#include "cli_args.hpp"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <thread>

#include "sketch_files.hpp"

namespace lashhost {
namespace {

const Option HELP = {"help", 0, false};

// by letter when there is one, else by name
const Option *lookup(const Command &cmd, const std::string &name, char letter)
{
    for (const Option &o : cmd.options)
        if (letter ? o.letter == letter : name == o.name) return &o;
    return !letter && name == HELP.name ? &HELP : nullptr;
}

bool to_u64(const std::string &s, uint64_t &v)
{
    if (s.empty()) return false;
    char *e = nullptr;
    v = strtoull(s.c_str(), &e, 10);
    return e && *e == 0 && s[0] != '-';
}

}  // namespace

bool Args::parse(int argc, char **argv, const Command &cmd)
{
    const auto long_name = [](const std::string &s) { return s.substr(2, s.find('=') == std::string::npos ? std::string::npos : s.find('=') - 2); };
    if (cmd.closed)                                        // before anything else, and also where a --name stands as a value
        for (int i = 2; i < argc; ++i) {
            const std::string s = argv[i];
            if (s.rfind("--", 0) != 0 || lookup(cmd, long_name(s), 0)) continue;
            fprintf(stderr, "error: unexpected argument '--%s'\n", long_name(s).c_str());
            return false;
        }
    for (int i = 2; i < argc; ++i) {
        const std::string s = argv[i];
        std::string key, val;
        bool has_val = false;
        const Option *o = nullptr;
        if (s.rfind("--", 0) == 0) {
            key = long_name(s);
            if (s.find('=') != std::string::npos) { val = s.substr(s.find('=') + 1); has_val = true; }
            o = lookup(cmd, key, 0);                       // an open set takes an unknown --name with a value
        } else if (s.size() >= 2 && s[0] == '-' && (o = lookup(cmd, "", s[1]))) {
            key = o->name;
            if (s.size() > 2) { val = s.substr(2); has_val = true; }
        } else { fprintf(stderr, "error: unexpected argument '%s'\n", s.c_str()); return false; }
        if (o && !o->takes_value) { flags[key] = true; continue; }
        if (!has_val) {
            if (i + 1 >= argc) { fprintf(stderr, "error: a value is required for '--%s'\n", key.c_str()); return false; }
            val = argv[++i];
        }
        kv[key] = val;
    }
    return true;
}

bool Args::invalid(const char *name) const
{
    fprintf(stderr, "error: invalid value for --%s\n", name);
    return false;
}

bool Args::invalid(const char *name, const std::string &required) const
{
    fprintf(stderr, "error: invalid value '%s' for --%s: %s\n", str(name).c_str(), name, required.c_str());
    return false;
}

bool Args::u64(const char *name, uint64_t &v) const
{
    return !kv.count(name) || to_u64(kv.at(name), v) || invalid(name);
}

bool Args::u64(const char *name, uint64_t &v, uint64_t lo, uint64_t hi, const std::string &required) const
{
    return !kv.count(name) || (to_u64(kv.at(name), v) && v >= lo && v <= hi) || invalid(name, required);
}

bool Args::real(const char *name, double &v, bool (*ok)(double), const std::string &required) const
{
    if (!kv.count(name)) return true;
    const std::string &s = kv.at(name);
    char *e = nullptr;
    const double d = s.empty() ? NAN : strtod(s.c_str(), &e);
    if (!e || *e != 0 || !(ok ? ok(d) : std::isfinite(d))) return invalid(name, required);
    v = d;
    return true;
}

bool Args::choice(const char *name, std::initializer_list<const char *> words, int &index, const char *required) const
{
    if (!kv.count(name)) return true;
    const auto at = std::find(words.begin(), words.end(), kv.at(name));
    if (at == words.end()) return required ? invalid(name, required) : false;
    index = (int)(at - words.begin());
    return true;
}

bool Args::u64_list(const char *name, std::vector<uint64_t> &out, uint64_t lo, uint64_t hi) const
{
    if (!kv.count(name)) return true;
    const std::string &l = kv.at(name);
    size_t at = 0;
    while (at <= l.size()) {
        const size_t c = l.find(',', at);
        uint64_t v = 0;
        if (!to_u64(l.substr(at, c == std::string::npos ? std::string::npos : c - at), v) || v < lo || v > hi) return false;
        out.push_back(v);
        if (c == std::string::npos) break;
        at = c + 1;
    }
    return true;
}

bool Args::require(std::initializer_list<std::pair<const char *, const char *>> rows, bool all_lines) const
{
    std::string lines;
    bool missing = false;
    for (const auto &r : rows) {
        missing = missing || !kv.count(r.first);
        if (all_lines || !kv.count(r.first)) lines += std::string("  --") + r.first + " <" + r.second + ">\n";
    }
    if (missing) fprintf(stderr, "error: the following required arguments were not provided:\n%s", lines.c_str());
    return !missing;
}

bool Args::allowed(const char *name, std::initializer_list<Rule> rules) const
{
    if (!has(name)) return true;
    for (const Rule &r : rules) {
        if (!(r.other ? has(r.other) : r.hit)) continue;
        if (r.other) fprintf(stderr, "error: --%s cannot be used with --%s (%s)\n", name, r.other, r.text.c_str());
        else fprintf(stderr, "error: --%s %s\n", name, r.text.c_str());
        return false;
    }
    return true;
}

bool devices_option(const Args &a, std::vector<int> &devices)
{
    std::vector<uint64_t> list;
    if (!a.u64_list("devices", list)) return a.invalid("devices");
    for (uint64_t d : list) devices.push_back((int)d);
    return true;
}

bool bias_source(const Args &a, DistOptions &side)
{
    side.hll_bias_sim = a.has("hll-bias-sim");
    if (!a.allowed("hll-bias-sim", {{"hll-bias", "simulate the tables or read them from a file, not both"}})) return false;
    if (a.has("hll-bias")) side.hll_bias_file = a.str("hll-bias");
    else if (const char *e = side.hll_bias_sim ? nullptr : getenv("LASH_HLL_BIAS")) side.hll_bias_file = e;
    return true;
}

bool threads_device_order(const Args &a, DistOptions &side)
{
    uint64_t threads = std::thread::hardware_concurrency(), dev = 0;
    if (!a.u64("threads", threads) || !a.u64("device", dev)) return false;
    side.threads = (int)std::max<uint64_t>(1, threads);
    side.device = (int)dev;
    side.file_order = a.has("file-order");
    return true;
}

bool layout_option(const Args &a, lash_layout &layout)
{
    const std::string err = layout_from_option(a.str("layout"), layout);
    if (!err.empty()) fprintf(stderr, "error: %s\n", err.c_str());
    return err.empty();
}

bool groups_or_all(const Args &a, bool required, std::string &groups_file, std::string &all_name)
{
    if (!a.allowed("groups", {{"all", "a list of groups or one group of everything, not both"}})) return false;
    if (required && !a.has("groups") && !a.has("all")) { fprintf(stderr, "error: one of --groups <file> and --all <name> is required\n"); return false; }
    if (!a.allowed("keep-others", {{"all", "--all leaves no others"}})) return false;       // (merge alone has --keep-others)
    if (a.has("all") && a.str("all").empty()) return a.invalid("all", "a name is required");
    if (a.has("groups")) groups_file = a.str("groups");
    if (a.has("all")) all_name = a.str("all");
    return true;
}

int finish(const std::string &err, const char *done)
{
    if (!err.empty()) { fprintf(stderr, "Error: %s\n", err.c_str()); return 1; }
    printf("%s", done);
    return 0;
}

}  // namespace lashhost
