"""`tracs threshold` -- estimate the SNP threshold that separates recent transmission from background diversity.

Interface and model follow /root/reference/tracs/threshold.py: flags :12-53, the negative binomial of the distant pairs :56-60, 88-92,
the Poisson + negative binomial mixture of the close pairs :63-67, 95-99, the threshold :103.  Two deliberate deviations
(INTEGRATION.md): the mixture's log-likelihood is MAXIMISED (the reference hands +sum(log-likelihood) to a minimiser), and the
results are written to -o (the reference takes -o and only logs).

The fit runs on (value, count) pairs -- sum(c * logpmf(v)) -- so the input can be the histogram `tracs distance --histogram` counts on
the GPU (--histogram) as well as the reference's two CSV files (--close / --distant), which are reduced to counts while they are read.
SciPy is imported by this command only.
"""
import logging
import os
import re

PARAMETERS = ("r", "p", "q", "lambda", "snp_threshold", "n_close", "n_distant", "converged")


def threshold_parser(parser):
    parser.description = "Estimates transmission thresholds."
    io = parser.add_argument_group("Input/output")
    io.add_argument("--close", dest="close_file", default=None, type=os.path.abspath,
                    help="path to csv file with distances between isolates mostly linked by recent transmission")
    io.add_argument("--distant", dest="distant_file", default=None, type=os.path.abspath,
                    help="path to csv file with distances between isolates not related by recent transmission")
    io.add_argument("--histogram", dest="histogram_file", default=None, type=os.path.abspath,
                    help="instead of --close / --distant: the output of `tracs distance --histogram --groups ...`; pairs within a "
                         "group are the close sample, pairs between groups the distant one (not in the reference)")
    io.add_argument("--which", dest="which", default="snp", type=str,
                    help="with --histogram: the column block to fit, snp or filter (default=snp)")
    io.add_argument("-o", "--output", dest="output_file", required=True, type=os.path.abspath, help="location of an output file")
    io.add_argument("--column", dest="column", default=1, type=int, help="index of column containing SNP distances (default=1)")
    parser.set_defaults(func=threshold)
    return parser


def check_threshold_args(args):
    """Which input is given (SystemExit with the message otherwise)."""
    hist = getattr(args, "histogram_file", None)
    close, distant = getattr(args, "close_file", None), getattr(args, "distant_file", None)
    if hist is not None:
        if close is not None or distant is not None:
            raise SystemExit("tracs threshold: --histogram replaces --close and --distant; give one or the other")
        if args.which not in ("snp", "filter"):
            raise SystemExit("tracs threshold: --which must be snp or filter, got '%s'" % args.which)
    elif close is None or distant is None:
        raise SystemExit("tracs threshold: give --close and --distant, or --histogram")


_COUNT = re.compile(r"\d+(\.0+)?\Z")


def _as_count(text):
    """'3' or '3.0' -> 3; anything else (a sign, an exponent, a fraction, no number) -> ValueError."""
    t = text.strip()
    if not _COUNT.match(t):
        raise ValueError(t)
    return int(t.split(".")[0])


def read_distance_column(path, column):
    """A csv with a header line, the distance in field `column` -> {value: count}.  Values must be non-negative integers."""
    counts = {}
    with open(path, "r") as fh:
        next(fh, None)
        for ln, line in enumerate(fh, 2):
            line = line.rstrip("\r\n")
            if not line:
                continue
            f = line.split(",")
            try:
                v = _as_count(f[column])
            except (ValueError, IndexError):
                raise SystemExit("tracs threshold: %s line %d: column %d does not hold a non-negative integer distance%s"
                                 % (path, ln, column, (" ('%s')" % f[column].strip()) if -len(f) <= column < len(f) else " (no such column)"))
            counts[v] = counts.get(v, 0) + 1
    return counts


def read_histogram(path, which):
    """A `tracs distance --histogram` file -> ({value: count} of `within`, the same of `between`, the MSA file values seen), counts
    summed over the MSA files, rows of the column block `which` only."""
    close, distant, refs = {}, {}, []
    with open(path, "r") as fh:
        next(fh, None)
        for ln, line in enumerate(fh, 2):
            line = line.rstrip("\r\n")
            if not line:
                continue
            f = line.split(",", 5)
            try:
                if len(f) != 6:
                    raise ValueError(line)
                v, w, b = _as_count(f[1]), _as_count(f[2]), _as_count(f[3])
                _as_count(f[4])
            except ValueError:
                raise SystemExit("tracs threshold: %s line %d is not a histogram row (column,distance,within,between,ungrouped,MSA file)"
                                 % (path, ln))
            if f[0] != which:
                continue
            if f[5] not in refs:
                refs.append(f[5])
            if w:
                close[v] = close.get(v, 0) + w
            if b:
                distant[v] = distant.get(v, 0) + b
    return close, distant, refs


def fit(close, distant):
    """close, distant: {value: count} (or (values, counts)) -> dict of PARAMETERS.  (i) r, p: Nelder-Mead (SciPy defaults) from
    (100, 0.5) on -sum(c * nbinom.logpmf(v; r, p)) over the distant sample; (ii) q, lambda: Nelder-Mead from (0.5, 1) on
    -sum(c * logsumexp(log q + poisson.logpmf(v; lambda), log(1 - q) + nbinom.logpmf(v; r, p))) over the close sample;
    (iii) snp_threshold = 3 * poisson.ppf(0.95, lambda)."""
    import numpy as np
    import scipy.optimize as optimize
    from scipy import stats
    from scipy.special import logsumexp

    def arrays(h):
        if isinstance(h, dict):
            v = np.array(sorted(h), dtype=np.float64)
            c = np.array([h[k] for k in sorted(h)], dtype=np.float64)
        else:
            v, c = np.asarray(h[0], dtype=np.float64), np.asarray(h[1], dtype=np.float64)
        keep = c > 0
        return v[keep], c[keep]
    cv, cc = arrays(close)
    dv, dc = arrays(distant)
    if not len(cv) or not len(dv):
        raise ValueError("fit(): the close and the distant sample must both hold pairs")

    def negbinom_ll(params):
        r, p = params
        if r <= 0 or p <= 0 or p >= 1:
            return np.inf
        return -np.sum(dc * stats.nbinom.logpmf(dv, r, p))
    far = optimize.minimize(negbinom_ll, np.array([100, 0.5]), method="nelder-mead")
    r, p = far.x
    nb_close = stats.nbinom.logpmf(cv, r, p)

    def mixture(params):
        q, lambd = params
        if q <= 0 or q >= 1 or lambd <= 0:
            return np.inf
        a = np.log(q) + stats.poisson.logpmf(cv, mu=lambd)
        b = np.log(1 - q) + nb_close
        return -np.sum(cc * logsumexp([a, b], axis=0))
    mix = optimize.minimize(mixture, np.array([0.5, 1]), method="nelder-mead")
    q, lambd = mix.x
    return {"r": float(r), "p": float(p), "q": float(q), "lambda": float(lambd),
            "snp_threshold": float(stats.poisson.ppf(0.95, mu=lambd) * 3),
            "n_close": int(round(float(cc.sum()))), "n_distant": int(round(float(dc.sum()))),
            "converged": bool(far.success and mix.success)}


def write_result(path, res):
    with open(path, "w") as out:
        out.write("parameter,value\n")
        for k in PARAMETERS:
            out.write("%s,%s\n" % (k, repr(res[k])))


def threshold(args):
    check_threshold_args(args)
    logging.basicConfig(format="%(asctime)s - %(message)s", datefmt="%d-%b-%y %H:%M:%S", level=logging.INFO)
    logging.info("Loading distances...")
    if args.histogram_file is not None:
        close, distant, refs = read_histogram(args.histogram_file, args.which)
        logging.info("Summed the '%s' rows of %d MSA file(s): %s", args.which, len(refs), ", ".join(refs))
        for name, h in (("within", close), ("between", distant)):
            if not h:
                raise SystemExit("tracs threshold: %s has no pairs in the '%s' column of its '%s' rows; run `tracs distance --histogram` "
                                 "with --groups so that pairs within and between groups are told apart"
                                 % (args.histogram_file, name, args.which))
    else:
        close = read_distance_column(args.close_file, args.column)
        distant = read_distance_column(args.distant_file, args.column)
        for name, path, h in (("--close", args.close_file, close), ("--distant", args.distant_file, distant)):
            if not h:
                raise SystemExit("tracs threshold: %s %s holds no distances" % (name, path))
    logging.info("Fitting distribution...")
    res = fit(close, distant)
    logging.info("Fitted parameters - r:%s, p:%s, q:%s, lambda:%s" % (res["r"], res["p"], res["q"], res["lambda"]))
    logging.info("SNP threshold: %s" % res["snp_threshold"])
    write_result(args.output_file, res)
    return res
