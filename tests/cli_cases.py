"""The command lines whose exit code, stdout and stderr tests/golden/cli_surface.json records (tools/record_cli_surface.py) and
tests/test_cli_surface.py compares.  CASES is a plain list of argument lists, without the program.  Every case ends before a GPU
is touched: it is refused (exit 2 or 101), it is --help, or it is accepted and fails on an input that is not there (the cases run
in an empty directory).  So there is no accepted `hll-bias` case: that command reads nothing before it opens the device."""

CASES = []


def case(*args):
    if list(args) not in CASES:                    # (the loops below meet some lines twice)
        CASES.append(list(args))


def forms(base, options):
    """one line per spelling, each with all of (long, letter, value): -x v, -xv, --long v, --long=v (no letter: the long spelling)"""
    case(*base, *[w for long, x, v in options for w in (["-" + x, v] if x else ["--" + long, v])])
    case(*base, *[w for long, x, v in options for w in (["-" + x + v] if x else ["--" + long + "=" + v])])
    case(*base, *[w for long, x, v in options for w in ("--" + long, v)])
    case(*base, *["--" + long + "=" + v for long, x, v in options])


def both(base, one, other):
    """two groups of arguments in both orders"""
    case(*base, *one, *other)
    case(*base, *other, *one)


SKETCH = ["sketch", "-f", "missing.txt"]           # accepted: exit 1, the list file cannot be opened
DIST = ["dist", "-q", "none", "-r", "none"]        # accepted: exit 1, "There should be 3 files starting with none"
GROWTH = ["growth", "-r", "none"]
MERGE = ["merge", "-r", "none", "-o", "out"]
SPECTRUM = ["spectrum", "-r", "none", "-o", "out"]
SCREEN = ["screen", "-r", "none", "-q", "none", "-o", "out.tsv"]
BIAS = ["hll-bias", "-o", "bias.txt"]
COMMANDS = ["sketch", "dist", "growth", "merge", "spectrum", "screen", "hll-bias"]
CLOSED = {"growth": GROWTH, "merge": MERGE + ["--all", "x"], "spectrum": SPECTRUM, "screen": SCREEN}

# ---- help and top level (the logger banner on stdout is part of every record)
case()
for word in ("--help", "-h", "help", "-V", "--version", "nonsense"):
    case(word)
for cmd in COMMANDS:
    case(cmd, "--help")
    case(cmd)                                      # nothing at all: the required arguments
case("dist", "--help=yes")                         # a flag given a value is still the flag
case("sketch", "-k", "x", "--help")                # --help is answered before any value is looked at
case("merge", "--help", "--bogus")                 # ... but not before the closed sets' scan
case("sketch", "-h")                               # -h is a letter no command has

# ---- option forms: every option of every command in each spelling it has (a line that is accepted took every one of them)
forms(["sketch"], [("file", "f", "missing.txt"), ("output", "o", "pre"), ("kmer", "k", "21"), ("threads", "t", "2"), ("algorithm", "a", "ull"),
                   ("precision", "p", "12"), ("seed", "s", "7"), ("min-count", "", "2"), ("count-cells-log2", "", "20"), ("gpus", "", "2"),
                   ("device", "", "1"), ("devices", "", "0,1"), ("batch-mb", "", "8"), ("stream-mb", "", "16"), ("layout", "", "kmer=lsb")])
forms(SKETCH, [("window", "", "1000")])
for flag in ("hmh-x-low", "per-record", "aa", "translate"):
    case(*SKETCH, "-k", "11", "--" + flag)
case(*SKETCH, "-k", "11", "--aa=1")
forms(["dist"], [("query", "q", "none"), ("reference", "r", "none"), ("output_file", "o", "out.tsv"), ("threads", "t", "2"), ("estimator", "e", "ml"),
                 ("model", "m", "0"), ("block-rows", "", "3"), ("device", "", "1"), ("devices", "", "0,0"), ("max-dist", "", "0.1"), ("top", "", "3"),
                 ("containment", "", "query"), ("hll-bias", "", "bias.txt"), ("layout", "", "kmer=lsb")])
forms(DIST, [("cluster", "", "0.05"), ("linkage", "", "complete")])
for mode in (["--derep", "0.05"], ["--derep=0.05"], ["--pcoa", "3"], ["--pcoa=3"], ["--tree", "--nj"], ["--tree=1"],
             ["--fp32", "--dm", "--file-order", "--hll-bias-sim"]):
    case(*DIST, *mode)
forms(["growth"], [("reference", "r", "none"), ("output_file", "o", "g.tsv"), ("threads", "t", "2"), ("estimator", "e", "ml"), ("orders", "", "3"),
                   ("seed", "", "7"), ("device", "", "1"), ("hll-bias", "", "bias.txt"), ("layout", "", "kmer=lsb")])
case(*GROWTH, "--file-order", "--hll-bias-sim")
forms(["merge"], [("reference", "r", "none"), ("output", "o", "out"), ("threads", "t", "2"), ("groups", "", "g.tsv"), ("device", "", "1"),
                  ("layout", "", "kmer=lsb")])
forms(MERGE, [("all", "", "x")])
case(*MERGE, "--groups", "g.tsv", "--keep-others", "--file-order")
forms(["spectrum"], [("reference", "r", "none"), ("output", "o", "out"), ("threads", "t", "2"), ("groups", "", "g.tsv"), ("core", "", "0.9"),
                     ("cloud", "", "0.1"), ("device", "", "1"), ("layout", "", "kmer=lsb")])
forms(SPECTRUM, [("all", "", "x")])
case(*SPECTRUM, "--curves", "--file-order")
forms(["screen"], [("reference", "r", "none"), ("query", "q", "none"), ("output", "o", "out.tsv"), ("threads", "t", "2"), ("model", "m", "0"),
                   ("max-dist", "", "0.05"), ("block-rows", "", "3"), ("device", "", "1"), ("layout", "", "kmer=lsb")])
case(*SCREEN, "--keep-losers", "--file-order")
# hll-bias: refused cases only, so its forms end in the last value it looks at, and that one is bad
forms(["hll-bias"], [("output", "o", "bias.txt"), ("precision", "p", "4,5"), ("points", "", "100"), ("trials", "", "16"), ("seed", "", "7"),
                     ("device", "", "x")])

# ---- a value missing at the end of the line, a stray positional, an unknown short letter
for cmd in COMMANDS:
    case(cmd, "-o")
    case(cmd, "stray")
    case(cmd, "-z")
    case(cmd, "-zvalue")
    case(cmd, "--")
case("sketch", "-")
case("sketch", "--", "value")
case("dist", "--=value")
case(*SKETCH, "--window")
case(*SKETCH, "stray")
case(*DIST, "--top")
case(*DIST, "stray", "--dm")
case(*GROWTH, "--orders")
case(*MERGE, "--all")
case(*SCREEN, "--max-dist")
case("hll-bias", "-p")
case("dist", "-q", "none", "-r")
case("sketch", "-q", "none")                       # a letter of another command
case("merge", "-q", "none")
case("hll-bias", "-r", "none")

# ---- open and closed option sets
case(*SKETCH, "--whatever", "value")               # sketch, dist and hll-bias take an unknown --option and its value in silence
case(*SKETCH, "--whatever=value")
case(*SKETCH, "--whatever")
case("sketch", "--whatever", "-f", "missing.txt")  # ... the value being whatever comes next
case(*DIST, "--whatever", "value")
case(*DIST, "--whatever")
case(*DIST, "--whatever", "--dm", "--top", "3")    # (--dm is the value here, so --top stands)
case(*DIST, "--keep-losers", "--dm", "--top", "3")
case("hll-bias", "--whatever", "value")
case("hll-bias", "--whatever")
for cmd, base in CLOSED.items():
    case(*base, "--whatever", "value")
    case(*base, "--whatever=value")
    case(*base, "-t", "--whatever")                # refused also where it stands as another option's value
    case(cmd, "stray", "--dm")                     # the scan reports before any other parse error
    case(*base, "--threads", "x", "--bogus")       # ... and before any value is looked at
    case(*base, "--top", "3")
case("merge", "-o", "--x")
case(*GROWTH, "-q", "none")
case(*GROWTH, "--devices", "0,0")
case(*MERGE, "--all", "x", "--core", "0.9")
case(*MERGE, "--all", "x", "-e", "ml")
case(*SPECTRUM, "--keep-others")
case(*SPECTRUM, "--hll-bias-sim")
case(*SCREEN, "--keep-others")
case(*SCREEN, "-e", "ml")
case(*SCREEN, "--containment", "query")

# ---- required arguments: dist names both whichever is missing, the newer commands only what is missing
case("dist", "-q", "none")
case("dist", "-r", "none")
case("dist", "--top", "abc")                       # required arguments come before values
case("sketch", "-k", "x")
case("growth", "--orders", "x")
case("merge", "-r", "none")
case("merge", "-o", "out")
case("merge", "--groups", "g", "--all", "x")       # ... and before the groups / all pair
case("spectrum", "-r", "none")
case("spectrum", "-o", "out", "--core", "7")
case("screen", "-r", "none")
case("screen", "-q", "none")
case("screen", "-o", "out.tsv")
case("screen", "-r", "none", "-q", "none")
case("screen", "-q", "none", "-o", "out.tsv", "--max-dist", "7")
case("hll-bias", "-p", "99")

# ---- the terse "invalid value for --x": what is no unsigned integer is refused (the kinds of it in turn), zero passes
TERSE = [(SKETCH, ["kmer", "precision", "seed", "threads", "gpus", "device", "batch-mb", "stream-mb"]),
         (DIST, ["block-rows", "model", "threads", "device"]),
         (GROWTH, ["seed", "threads", "device"]),
         (MERGE + ["--all", "x"], ["threads", "device"]),
         (SPECTRUM, ["threads", "device"]),
         (SCREEN, ["block-rows", "threads", "device"]),
         (BIAS, ["seed", "device"])]
n = 0
for base, names in TERSE:
    for name in names:
        case(*base, "--" + name, ("x", "-1", "", "1.5")[n % 4])
        n += 1
        if base is not BIAS and name != "kmer":    # (accepted values: not for hll-bias, which would go on to the device; -k: below)
            case(*base, "--" + name, "0")
for value in ("x", "-1", "", "1.5", "7x", "1 "):
    case(*SKETCH, "--seed", value)
for value in ("+1", " 1", "18446744073709551615", "18446744073709551616"):    # a sign, white space and 2^64 pass
    case(*SKETCH, "--seed", value)
    case(*DIST, "--block-rows", value)
case(*SKETCH, "-k", "x", "-p", "x")                # the first in the command's own order wins, not the first on the line
case(*SKETCH, "-p", "x", "-k", "x")
case(*SKETCH, "--stream-mb", "x", "--threads", "x")
case(*DIST, "--device", "x", "--block-rows", "x")
case(*DIST, "-t", "x", "-m", "x")
case(*GROWTH, "--device", "x", "--seed", "x")
case(*SCREEN, "--device", "x", "--block-rows", "x")
case(*BIAS, "--device", "x", "--seed", "x")
case(*DIST, "-m", "2")                             # dist takes any integer as the model here and refuses it after the files
case(*DIST, "-e", "bogus")

# ---- comma lists
for value in ("0,x", "", "0,", ",0", "0,,1", "0,-1", "0", "0,1,2,3"):
    case(*SKETCH, "--devices", value)
for value in ("0,x", "", "0,0"):
    case(*DIST, "--devices", value)
case(*SKETCH, "--devices", "0,1", "--gpus", "3", "--device", "2")
case(*SKETCH, "--devices", "x", "--gpus", "x")     # --gpus is looked at first
for value in ("3", "19", "x", "", "4,", "4,x", "4,4", "4,5,4", "4,4,99", "4,99,4"):
    case(*BIAS, "-p", value)
case(*BIAS, "-p", "18,4", "--points", "1")         # 4 and 18 pass: the next refusal shows it

# ---- the quoted "invalid value '..' for --x: ..": one bad value, and the boundary on each side
for value in ("x", "0", "1"):
    case(*SKETCH, "-k", "1", "--window", value)
case(*SKETCH, "--window", "15")                    # shorter than the default k
case(*SKETCH, "--window", "16")
case(*SKETCH, "-k", "21", "--window", "20")
for value in ("x", "", "0", "256", "1", "255"):
    case(*SKETCH, "--min-count", value)
for value in ("x", "9", "37", "10", "36"):
    case(*SKETCH, "--min-count", "2", "--count-cells-log2", value)
for name, values in (("top", ["x", "", "0", "1025", "2.5", "1", "1024"]),
                     ("pcoa", ["x", "0", "17", "-1", "1", "16"]),
                     ("max-dist", ["x", "", "nan", "inf", "0.5x", "1e999", "0", "-1", "7", " 0.5"]),
                     ("cluster", ["x", "nan", "-inf", "-1", "7"]),
                     ("derep", ["x", "nan", "inf", "-1", "7"]),
                     ("containment", ["x", "", "Query", "query", "reference"])):
    for value in values:
        case(*DIST, "--" + name, value)
for value in ("x", "", "Average", "average", "single", "complete"):
    case(*DIST, "--tree", "--linkage", value)
    case(*DIST, "--cluster", "0.1", "--linkage", value)
for value in ("x", "0", "4294967296", "1", "4294967295"):
    case(*GROWTH, "--orders", value)
for value in ("x", "", "FGRA", "fgra", "ml"):
    case(*GROWTH, "-e", value)
for value in ("x", "", "0", "1.0001", "nan", "0.5x"):
    case(*SPECTRUM, "--core", value)
    case(*SPECTRUM, "--cloud", value)
case(*SPECTRUM, "--core", "1e-9", "--cloud", "1e-9")
case(*SPECTRUM, "--core", "1", "--cloud", "1")
case(*SPECTRUM, "--core", "0.1", "--cloud", "0.2") # cloud above core
case(*SPECTRUM, "--cloud", "0.2", "--core", "0.1")
case(*SPECTRUM, "--core", "0.1")                   # ... also against the default
case(*SPECTRUM, "--core", "x", "--cloud", "x")     # --core is looked at first
case(*SPECTRUM, "--cloud", "x", "--core", "x")
for value in ("x", "", "nan", "inf", "-1e-9", "1.0001", "0.5x", "0", "1", "-0"):
    case(*SCREEN, "--max-dist", value)
for value in ("x", "", "2", "-1", "0", "1"):
    case(*SCREEN, "-m", value)
for value in ("x", "5", "4294967296"):
    case(*BIAS, "--points", value)
case(*BIAS, "--points", "6", "--trials", "0")      # 6 and 2^32 - 1 pass: the next refusal shows it
case(*BIAS, "--points", "4294967295", "--trials", "0")
for value in ("x", "1048577"):
    case(*BIAS, "--trials", value)
case(*BIAS, "--trials", "1", "--seed", "x")
case(*BIAS, "--trials", "1048576", "--seed", "x")
case(*BIAS, "-p", "x", "--points", "x")            # the command's own order: -p, points, trials, seed, device
case(*BIAS, "--trials", "x", "--points", "x")
case(*BIAS, "--seed", "x", "--trials", "x")

# ---- the panics of the reference (exit 101)
for value in ("bogus", "HMH", "", "hmh", "hll"):
    case(*SKETCH, "-a", value)
for value in ("0", "33", "1", "32"):
    case(*SKETCH, "-k", value)
for value in ("12", "13"):
    case(*SKETCH, "--aa", "-k", value)
    case(*SKETCH, "--translate", "-k", value)
case(*SKETCH, "--translate")
case(*SKETCH, "--aa")
case(*SKETCH, "-a", "bogus", "-k", "0")            # the algorithm is looked at before k ...
case(*SKETCH, "-a", "bogus", "-k", "x")            # ... but after every plain number
case(*SKETCH, "-k", "0", "--translate", "--aa")
case(*SKETCH, "-k", "33", "--window", "x")
case(*SKETCH, "--translate", "--per-record", "--aa", "-k", "13")
case(*SKETCH, "--per-record", "--aa", "-k", "13")  # the refusal of the pair before the panic of the k
case(*SKETCH, "--aa", "-k", "13", "--count-cells-log2", "20")
case(*SKETCH, "--translate", "--count-cells-log2", "20")
case(*SKETCH, "--aa", "-k", "13", "--min-count", "2")
case(*SKETCH, "--aa", "-k", "13", "--window", "20")

# ---- sketch: every "cannot be used with" and "needs" pair in both orders, and which of two refusals wins
K = ["-k", "11"]
both(SKETCH + K, ["--translate"], ["--aa"])
both(SKETCH + K, ["--translate"], ["--min-count", "2"])
both(SKETCH + K, ["--translate"], ["--window", "100"])
both(SKETCH + K, ["--window", "100"], ["--aa"])
both(SKETCH + K, ["--window", "100"], ["--min-count", "2"])
both(SKETCH + K, ["--per-record"], ["--aa"])
both(SKETCH + K, ["--min-count", "2"], ["--aa"])
both(SKETCH + K, ["--min-count", "2"], ["--per-record"])
both(SKETCH + K, ["--count-cells-log2", "20"], ["--aa"])
case(*SKETCH, "--count-cells-log2", "x")           # needs --min-count: the value is not looked at
both(SKETCH + K, ["--window", "100"], ["--per-record"])            # allowed together
both(SKETCH + K, ["--translate"], ["--per-record"])
case(*SKETCH, *K, "--translate", "--aa", "--min-count", "2", "--window", "100")
case(*SKETCH, *K, "--translate", "--min-count", "x", "--window", "x")
case(*SKETCH, *K, "--translate", "--window", "x")
case(*SKETCH, *K, "--window", "x", "--aa")                         # the value before the pair
case(*SKETCH, *K, "--window", "5", "--aa")                         # the pair before the length against k
case(*SKETCH, *K, "--window", "5", "--min-count", "2")             # the length against k before the next pair
case(*SKETCH, *K, "--window", "100", "--min-count", "x")           # the pair before the other option's value
case(*SKETCH, *K, "--window", "100", "--count-cells-log2", "20")
case(*SKETCH, *K, "--min-count", "x", "--aa")
case(*SKETCH, *K, "--min-count", "2", "--count-cells-log2", "x", "--aa")
case(*SKETCH, *K, "--min-count", "2", "--aa", "--per-record")
case(*SKETCH, *K, "--min-count", "2", "--per-record", "-a", "hll", "-p", "16")
case(*SKETCH, "--min-count", "2", "--layout", "bogus", "--devices", "x")
case(*SKETCH, "--layout", "bogus")
case(*SKETCH, "--layout", "")
case(*SKETCH, "--devices", "x", "--layout", "bogus")               # the layout is looked at before the list
for algo, p in (("hll", "15"), ("hll", "16"), ("ull", "14"), ("ull", "15"), ("hmh", "20")):
    case(*SKETCH, "--min-count", "2", "-a", algo, "-p", p)

# ---- dist: every "cannot be used with" and "needs" pair in both orders
MODES = {"dm": ["--dm"], "max-dist": ["--max-dist", "0.1"], "top": ["--top", "3"], "cluster": ["--cluster", "0.05"],
         "derep": ["--derep", "0.05"], "containment": ["--containment", "query"], "tree": ["--tree"],
         "linkage": ["--tree", "--linkage", "single"], "nj": ["--tree", "--nj"], "pcoa": ["--pcoa", "3"]}
for one, other in (("max-dist", "dm"), ("top", "dm"),
                   ("cluster", "dm"), ("cluster", "top"), ("cluster", "max-dist"),
                   ("derep", "dm"), ("derep", "top"), ("derep", "max-dist"), ("derep", "cluster"),
                   ("containment", "dm"), ("containment", "cluster"), ("containment", "derep"),
                   ("tree", "dm"), ("tree", "top"), ("tree", "max-dist"), ("tree", "cluster"), ("tree", "derep"), ("tree", "containment"),
                   ("nj", "cluster"), ("nj", "linkage"),
                   ("pcoa", "dm"), ("pcoa", "top"), ("pcoa", "max-dist"), ("pcoa", "cluster"), ("pcoa", "derep"), ("pcoa", "containment"),
                   ("pcoa", "tree"), ("pcoa", "nj"), ("pcoa", "linkage"),
                   ("max-dist", "top"), ("max-dist", "containment"), ("top", "containment")):       # (the last three go together)
    both(DIST, MODES[one], MODES[other])
both(DIST, ["--pcoa", "3"], ["--cluster", "0.05", "--linkage", "average"])
both(DIST, ["--nj"], ["--cluster", "0.05"])                        # --nj without --tree: the pair is named first
both(DIST, ["--nj"], ["--linkage", "single"])                      # (--linkage without --tree is refused before --nj is looked at)
case(*DIST, "--nj")
case(*DIST, "--linkage", "single")
case(*DIST, "--linkage", "x")                      # the value before what the option needs
both(DIST, ["--linkage", "complete"], ["--derep", "0.05"])
both(DIST, ["--derep", "0.05"], ["--devices", "0,1"])
both(DIST, ["--derep", "0.05"], ["--devices", "0"])
both(DIST, ["--hll-bias-sim"], ["--hll-bias", "bias.txt"])
both(GROWTH, ["--hll-bias-sim"], ["--hll-bias", "bias.txt"])
for flag in (["--tree"], ["--pcoa", "3"], ["--cluster", "0.05"], ["--derep", "0.05"]):
    case("dist", "-q", "a", "-r", "b", *flag)      # all-vs-all only; --cluster and --derep find out after the files
    case("dist", "-q", "dir/none", "-r", "./none", *flag)

# ---- dist: which refusal wins, a conflict or a later bad value, and which of two conflicts
case(*DIST, "--max-dist", "0.1", "--dm", "--top", "abc")           # the --dm conflict of --max-dist
case(*DIST, "--max-dist", "abc", "--dm", "--top", "abc")
case(*DIST, "--top", "3", "--dm", "--max-dist", "abc")             # --max-dist is looked at first wherever it stands
case(*DIST, "--top", "3", "--dm", "--cluster", "abc")
case(*DIST, "--top", "abc", "--cluster", "0.1", "--dm")
case(*DIST, "--cluster", "0.1", "--dm", "--top", "3", "--max-dist", "0.1")     # --max-dist against --dm
case(*DIST, "--cluster", "0.1", "--top", "3", "--max-dist", "0.1")             # --cluster: --top before --max-dist
case(*DIST, "--cluster", "0.1", "--top", "3", "--derep", "abc")
case(*DIST, "--cluster", "abc", "--derep", "abc", "--top", "3")
case(*DIST, "--derep", "0.1", "--cluster", "0.1", "--top", "3")                # --cluster's conflict with --top
case(*DIST, "--derep", "0.1", "--cluster", "0.1", "--containment", "x")
case(*DIST, "--derep", "0.1", "--max-dist", "0.1", "--cluster", "abc")
case(*DIST, "--derep", "0.1", "--devices", "0,1", "--cluster", "0.1")
case(*DIST, "--derep", "0.1", "--devices", "0,x", "--dm")
case(*DIST, "--derep", "0.1", "--devices", "0,1", "--pcoa", "x")
case(*DIST, "--containment", "query", "--cluster", "0.1", "--derep", "0.1")
case(*DIST, "--containment", "query", "--derep", "0.1", "--tree")
case(*DIST, "--containment", "x", "--dm", "--tree")
case(*DIST, "--containment", "query", "--dm", "--tree")
case(*DIST, "--containment", "query", "--tree", "--pcoa", "x")
case(*DIST, "--tree", "--dm", "--top", "3")                        # --top against --dm before anything of --tree
case(*DIST, "--tree", "--top", "3", "--max-dist", "0.1")
case(*DIST, "--tree", "--derep", "0.1", "--cluster", "0.1")
case(*DIST, "--tree", "--containment", "query", "--linkage", "x")
case(*DIST, "--tree", "--cluster", "0.1", "--linkage", "x")
case("dist", "-q", "a", "-r", "b", "--tree", "--containment", "query")         # a conflict before the all-vs-all check
case("dist", "-q", "a", "-r", "b", "--tree", "--linkage", "x")                 # ... which comes before the next option's value
case("dist", "-q", "a", "-r", "b", "--pcoa", "3", "--linkage", "single")
case("dist", "-q", "a", "-r", "b", "--pcoa", "0")
case(*DIST, "--linkage", "x", "--nj", "--cluster", "0.1")
case(*DIST, "--tree", "--nj", "--linkage", "single", "--cluster", "0.1")       # --tree against --cluster
case(*DIST, "--nj", "--linkage", "single", "--cluster", "0.1")                 # --nj against --cluster before --linkage
case(*DIST, "--nj", "--linkage", "single", "--pcoa", "3")
case(*DIST, "--tree", "--nj", "--pcoa", "x")
case(*DIST, "--pcoa", "3", "--tree", "--cluster", "0.1")                       # --tree against --cluster
case(*DIST, "--pcoa", "3", "--tree", "--nj", "--linkage", "single")            # --nj against --linkage
case(*DIST, "--pcoa", "3", "--dm", "--top", "3")
case(*DIST, "--pcoa", "3", "--top", "3", "--max-dist", "0.1")
case(*DIST, "--pcoa", "3", "--max-dist", "0.1", "--cluster", "0.1")
case(*DIST, "--pcoa", "3", "--derep", "0.1", "--containment", "query")
case(*DIST, "--pcoa", "x", "--dm")
case(*DIST, "--layout", "bogus")
case(*DIST, "--layout", "bogus", "--pcoa", "x")                    # the layout is looked at last
case(*DIST, "--hll-bias-sim", "--hll-bias", "bias.txt", "--devices", "x")
case(*DIST, "--hll-bias-sim", "--hll-bias", "bias.txt", "--device", "x")       # plain numbers before the bias tables
case(*DIST, "--devices", "x", "--max-dist", "abc")
case(*DIST, "--block-rows", "x", "--max-dist", "abc", "--dm")
case(*GROWTH, "--hll-bias-sim", "--hll-bias", "bias.txt", "--layout", "bogus")
case(*GROWTH, "--hll-bias-sim", "--hll-bias", "bias.txt", "--device", "x")
case(*GROWTH, "-e", "x", "--orders", "x")
case(*GROWTH, "--orders", "x", "--seed", "x")
case(*GROWTH, "--layout", "bogus")

# ---- merge and spectrum: a list of groups or one group of everything; the order of the shared tail
both(MERGE, ["--groups", "g.tsv"], ["--all", "x"])
both(SPECTRUM, ["--groups", "g.tsv"], ["--all", "x"])
both(MERGE, ["--all", "x"], ["--keep-others"])
case(*MERGE)
case(*MERGE, "--keep-others")
case(*MERGE, "--all", "")
case(*MERGE, "--all=")
case(*MERGE, "--all", "", "--keep-others")         # --keep-others is named before the empty name
case(*MERGE, "--all", "", "--groups", "g.tsv")
case(*MERGE, "--groups", "g.tsv", "--all", "x", "--keep-others")
case(*MERGE, "--groups", "")                       # an empty file name is the driver's to refuse
case(*MERGE, "--all", "", "-t", "x")
case(*MERGE, "-t", "x")                            # the pair before any number
case(*MERGE, "--all", "x", "-t", "x", "--device", "x")
case(*MERGE, "--all", "x", "--device", "x", "--layout", "bogus")
case(*MERGE, "--all", "x", "--layout", "bogus")
case(*SPECTRUM, "--all", "")
case(*SPECTRUM, "--all", "", "--groups", "g.tsv")
case(*SPECTRUM, "--all", "", "--core", "x")
case(*SPECTRUM, "--core", "x", "-t", "x")
case(*SPECTRUM, "--core", "0.1", "-t", "x")        # the fractions against each other before any number
case(*SPECTRUM, "-t", "x", "--device", "x")
case(*SPECTRUM, "--device", "x", "--layout", "bogus")
case(*SPECTRUM, "--layout", "bogus")
case(*SCREEN, "--max-dist", "x", "-m", "x")
case(*SCREEN, "-m", "x", "--block-rows", "x")
case(*SCREEN, "--block-rows", "x", "-t", "x")
case(*SCREEN, "-t", "x", "--device", "x")
case(*SCREEN, "--device", "x", "--layout", "bogus")
case(*SCREEN, "--layout", "bogus")

# ---- a repeated option: the last one counts
case(*SKETCH, "-k", "x", "-k", "21")
case(*SKETCH, "-k", "21", "--kmer=x")
case(*DIST, "--top", "abc", "--top", "3")
case(*DIST, "--top", "3", "--top=abc")
case(*DIST, "-q", "a", "-q", "none", "--tree")
