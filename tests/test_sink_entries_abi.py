"""What the byte sinks' entries refuse before an engine, a batch or a device is touched, by return code and
jb_last_error text: the 23 engine entries (per sink batch, batch_each, single and programme, for FLAC also the _meta
twins) and the batch-level size / read / read_all / set entries with a NULL handle.  Every call here passes NULL for
the engine (or the batch), so it never gets past the checks.  EXPECTED holds what the library returned before the
entries shared one shape; nothing in it is computed."""
import ctypes as C

import pytest

import jbonsai_amd as J
from jbonsai_amd import _ffi as F

GOOD_JOIN = F.join_opts(gap_ms=100.0)


def _reserved(o):
    o.reserved[0] = 1
    return o


# per sink: the option arguments that pass and, by name, the ones an entry refuses (None: a NULL pointer)
SINKS = {
    "flac": dict(good=(F.flac_opts(),), bad={"block_size": (F.flac_opts(block_size=5),)}, counts=False),
    "flac_meta": dict(good=(F.flac_opts(), F.flac_meta(md5=True)),
                      bad={"block_size": (F.flac_opts(block_size=5), None), "meta_flags": (None, F.FlacMeta(flags=2))},
                      counts=False),
    "formatted": dict(good=(F.format_opts("s16"),), bad={"format": (F.format_opts(9),), "null": (None,)}, counts=False),
    "adpcm": dict(good=(F.adpcm_opts(),), bad={"block_align": (F.adpcm_opts(30),), "null": (None,)}, counts=True),
    "fbank": dict(good=(F.fbank(),), bad={"n_mels": (F.fbank(n_mels=0),), "null": (None,)}, counts=True),
    "mfcc": dict(good=(F.fbank(), F.mfcc()),
                 bad={"n_mels": (F.fbank(n_mels=0), F.mfcc()), "n_ceps": (F.fbank(), F.mfcc(n_ceps=81)),
                      "null_fbank": (None, F.mfcc()), "null": (F.fbank(), None)}, counts=True),
}
# the entry families of each sink (FLAC has no programme entry without _meta)
FAMILIES = {s: ("batch", "batch_each", "single") + (("programme",) if s != "flac" else ()) for s in SINKS}
BAD_JOINS = {"null_join": None, "negative_gap": F.join_opts(gap_ms=-1.0), "reserved": _reserved(F.join_opts())}


def _ref(o):
    return None if o is None else C.byref(o)


def entry(sink, family, opts, join=GOOD_JOIN, n_utts=1, null_outputs=True):
    """(name, arguments) of one engine entry with NULL engine(s), lines and outputs around `opts` (and `join`); the
    single forms look at their output pointers first, so their option cases pass real ones"""
    opts = tuple(_ref(o) for o in opts)
    if null_outputs:
        outs = (None, None) + ((None,) if SINKS[sink]["counts"] else ())
    else:
        outs = (C.byref(C.POINTER(C.c_uint8)()), C.byref(C.c_size_t())) + ((None,) if SINKS[sink]["counts"] else ())
    if family == "single":
        return "jb_synthesize_" + sink, (None, None, 0) + opts + outs
    if family == "programme":
        return "jb_synthesize_programme_" + sink, (None, None, None, n_utts, -1) + opts + (_ref(join),) + outs + (None,)
    name = "jb_synthesize_batch_" + ("each_" if family == "batch_each" else "") + sink
    return name, (None, None, None, n_utts, -1) + opts + outs


def engine_cases():
    cases = {}
    for sink, s in SINKS.items():
        for family in FAMILIES[sink]:
            for what, opts in s["bad"].items():
                cases[f"{sink}-{family}-{what}"] = entry(sink, family, opts, null_outputs=family != "single")
            if family == "programme":
                for what, join in BAD_JOINS.items():
                    cases[f"{sink}-{family}-{what}"] = entry(sink, family, s["good"], join=join)
                cases[f"{sink}-{family}-no_utts"] = entry(sink, family, s["good"], n_utts=0)
            if family == "single":
                cases[f"{sink}-{family}-null_outputs"] = entry(sink, family, s["good"])
    return cases


def batch_cases():
    cases = {}
    for sink, size in (("flac", "flac_size"), ("formatted", "formatted_size"), ("adpcm", "adpcm_size"),
                       ("fbank", "fbank_size"), ("mfcc", "mfcc_size")):
        n = C.c_size_t()
        buf = (C.c_uint8 * 8)()
        # (the FLAC entries are bound with uint8_t pointers, the others with void pointers)
        u8p = C.POINTER(C.c_uint8)
        dst = buf if sink == "flac" else C.cast(buf, C.c_void_p)
        arr = (u8p * 1)(C.cast(buf, u8p)) if sink == "flac" else (C.c_void_p * 1)(C.addressof(buf))
        cases[f"{sink}-size"] = ("jb_batch_" + size, (None, 0, C.byref(n)))
        cases[f"{sink}-read"] = ("jb_batch_read_" + sink, (None, 0, dst, 8))
        cases[f"{sink}-read_all"] = (f"jb_batch_read_{sink}_all", (None, arr))
    cases["flac-set"] = ("jb_batch_set_flac", (None, C.byref(F.flac_opts())))
    cases["flac_meta-set"] = ("jb_batch_set_flac_meta", (None, C.byref(F.flac_meta(md5=True))))
    cases["formatted-set"] = ("jb_batch_set_format", (None, C.byref(F.format_opts("s16"))))
    cases["adpcm-set"] = ("jb_batch_set_adpcm", (None, C.byref(F.adpcm_opts())))
    cases["fbank-set"] = ("jb_batch_set_fbank", (None, C.byref(F.fbank())))
    cases["mfcc-set"] = ("jb_batch_set_mfcc", (None, C.byref(F.fbank()), C.byref(F.mfcc())))
    return cases


SENTINEL = "jb_synthesize_programme_i16: join is NULL"


def call(name, args):
    """(return code, the text the call set or None): before the call a refused PCM entry's text stands in jb_last_error"""
    lib = J.lib()
    assert lib.jb_synthesize_programme_i16(None, None, None, 0, -1, None, None, None, None) == -1
    assert lib.jb_last_error().decode() == SENTINEL
    rc = getattr(lib, name)(*args)
    text = lib.jb_last_error().decode()
    return rc, None if text == SENTINEL else text


ALIGN = "block_align is 0 (by the rate) or a multiple of 4 in 32..8192"
MS = "lead_ms, gap_ms, trail_ms and fade_ms are finite and not negative"
NO_UTTS = "a programme has at least one utterance"
FLAC_BLOCK = "jb_flac_opts: block_size must be 16..4608 (0: 4096)"
FLAC_FLAGS = "jb_flac_meta: unknown flag bits (JB_FLAC_MD5 is the only one)"
FORMAT = "a format is JB_FMT_F32, _S16, _S24, _ULAW or _ALAW"
N_CEPS = "n_ceps is at most n_mels (0: the log-mel energies themselves)"
# the single forms report under their batch form's name; the FLAC option checks name no entry
EXPECTED = {
    "adpcm-batch-block_align": (-1, "jb_synthesize_batch_adpcm: " + ALIGN),
    "adpcm-batch-null": (-1, "jb_synthesize_batch_adpcm: opts is NULL"),
    "adpcm-batch_each-block_align": (-1, "jb_synthesize_batch_each_adpcm: " + ALIGN),
    "adpcm-batch_each-null": (-1, "jb_synthesize_batch_each_adpcm: opts is NULL"),
    "adpcm-programme-block_align": (-1, "jb_synthesize_programme_adpcm: " + ALIGN),
    "adpcm-programme-negative_gap": (-1, "jb_synthesize_programme_adpcm: " + MS),
    "adpcm-programme-no_utts": (-1, "jb_synthesize_programme_adpcm: " + NO_UTTS),
    "adpcm-programme-null": (-1, "jb_synthesize_programme_adpcm: opts is NULL"),
    "adpcm-programme-null_join": (-1, "jb_synthesize_programme_adpcm: join is NULL"),
    "adpcm-programme-reserved": (-1, "jb_synthesize_programme_adpcm: reserved must be 0"),
    "adpcm-read": (-1, None),
    "adpcm-read_all": (-1, None),
    "adpcm-set": (-1, None),
    "adpcm-single-block_align": (-1, "jb_synthesize_batch_adpcm: " + ALIGN),
    "adpcm-single-null": (-1, "jb_synthesize_batch_adpcm: opts is NULL"),
    "adpcm-single-null_outputs": (-1, None),
    "adpcm-size": (-1, None),
    "fbank-batch-n_mels": (-1, "jb_synthesize_batch_fbank: n_mels is in 1..128"),
    "fbank-batch-null": (-1, "jb_synthesize_batch_fbank: opts is NULL"),
    "fbank-batch_each-n_mels": (-1, "jb_synthesize_batch_each_fbank: n_mels is in 1..128"),
    "fbank-batch_each-null": (-1, "jb_synthesize_batch_each_fbank: opts is NULL"),
    "fbank-programme-n_mels": (-1, "jb_synthesize_programme_fbank: n_mels is in 1..128"),
    "fbank-programme-negative_gap": (-1, "jb_synthesize_programme_fbank: " + MS),
    "fbank-programme-no_utts": (-1, "jb_synthesize_programme_fbank: " + NO_UTTS),
    "fbank-programme-null": (-1, "jb_synthesize_programme_fbank: opts is NULL"),
    "fbank-programme-null_join": (-1, "jb_synthesize_programme_fbank: join is NULL"),
    "fbank-programme-reserved": (-1, "jb_synthesize_programme_fbank: reserved must be 0"),
    "fbank-read": (-1, None),
    "fbank-read_all": (-1, None),
    "fbank-set": (-1, None),
    "fbank-single-n_mels": (-1, "jb_synthesize_batch_fbank: n_mels is in 1..128"),
    "fbank-single-null": (-1, "jb_synthesize_batch_fbank: opts is NULL"),
    "fbank-single-null_outputs": (-1, None),
    "fbank-size": (-1, None),
    "flac-batch-block_size": (-1, FLAC_BLOCK),
    "flac-batch_each-block_size": (-1, FLAC_BLOCK),
    "flac-read": (-1, None),
    "flac-read_all": (-1, None),
    "flac-set": (-1, None),
    "flac-single-block_size": (-1, FLAC_BLOCK),
    "flac-single-null_outputs": (-1, None),
    "flac-size": (-1, None),
    "flac_meta-batch-block_size": (-1, FLAC_BLOCK),
    "flac_meta-batch-meta_flags": (-1, FLAC_FLAGS),
    "flac_meta-batch_each-block_size": (-1, FLAC_BLOCK),
    "flac_meta-batch_each-meta_flags": (-1, FLAC_FLAGS),
    "flac_meta-programme-block_size": (-1, FLAC_BLOCK),
    "flac_meta-programme-meta_flags": (-1, FLAC_FLAGS),
    "flac_meta-programme-negative_gap": (-1, "jb_synthesize_programme_flac_meta: " + MS),
    "flac_meta-programme-no_utts": (-1, "jb_synthesize_programme_flac_meta: " + NO_UTTS),
    "flac_meta-programme-null_join": (-1, "jb_synthesize_programme_flac_meta: join is NULL"),
    "flac_meta-programme-reserved": (-1, "jb_synthesize_programme_flac_meta: reserved must be 0"),
    "flac_meta-set": (-1, None),
    "flac_meta-single-block_size": (-1, FLAC_BLOCK),
    "flac_meta-single-meta_flags": (-1, FLAC_FLAGS),
    "flac_meta-single-null_outputs": (-1, None),
    "formatted-batch-format": (-1, "jb_synthesize_batch_formatted: " + FORMAT),
    "formatted-batch-null": (-1, "jb_synthesize_batch_formatted: opts is NULL"),
    "formatted-batch_each-format": (-1, "jb_synthesize_batch_each_formatted: " + FORMAT),
    "formatted-batch_each-null": (-1, "jb_synthesize_batch_each_formatted: opts is NULL"),
    "formatted-programme-format": (-1, "jb_synthesize_programme_formatted: " + FORMAT),
    "formatted-programme-negative_gap": (-1, "jb_synthesize_programme_formatted: " + MS),
    "formatted-programme-no_utts": (-1, "jb_synthesize_programme_formatted: " + NO_UTTS),
    "formatted-programme-null": (-1, "jb_synthesize_programme_formatted: opts is NULL"),
    "formatted-programme-null_join": (-1, "jb_synthesize_programme_formatted: join is NULL"),
    "formatted-programme-reserved": (-1, "jb_synthesize_programme_formatted: reserved must be 0"),
    "formatted-read": (-1, None),
    "formatted-read_all": (-1, None),
    "formatted-set": (-1, None),
    "formatted-single-format": (-1, "jb_synthesize_batch_formatted: " + FORMAT),
    "formatted-single-null": (-1, "jb_synthesize_batch_formatted: opts is NULL"),
    "formatted-single-null_outputs": (-1, None),
    "formatted-size": (-1, None),
    "mfcc-batch-n_ceps": (-1, "jb_synthesize_batch_mfcc: " + N_CEPS),
    "mfcc-batch-n_mels": (-1, "jb_synthesize_batch_mfcc: n_mels is in 1..128"),
    "mfcc-batch-null": (-1, "jb_synthesize_batch_mfcc: the cepstral opts are NULL"),
    "mfcc-batch-null_fbank": (-1, "jb_synthesize_batch_mfcc: opts is NULL"),
    "mfcc-batch_each-n_ceps": (-1, "jb_synthesize_batch_each_mfcc: " + N_CEPS),
    "mfcc-batch_each-n_mels": (-1, "jb_synthesize_batch_each_mfcc: n_mels is in 1..128"),
    "mfcc-batch_each-null": (-1, "jb_synthesize_batch_each_mfcc: the cepstral opts are NULL"),
    "mfcc-batch_each-null_fbank": (-1, "jb_synthesize_batch_each_mfcc: opts is NULL"),
    "mfcc-programme-n_ceps": (-1, "jb_synthesize_programme_mfcc: " + N_CEPS),
    "mfcc-programme-n_mels": (-1, "jb_synthesize_programme_mfcc: n_mels is in 1..128"),
    "mfcc-programme-negative_gap": (-1, "jb_synthesize_programme_mfcc: " + MS),
    "mfcc-programme-no_utts": (-1, "jb_synthesize_programme_mfcc: " + NO_UTTS),
    "mfcc-programme-null": (-1, "jb_synthesize_programme_mfcc: the cepstral opts are NULL"),
    "mfcc-programme-null_fbank": (-1, "jb_synthesize_programme_mfcc: opts is NULL"),
    "mfcc-programme-null_join": (-1, "jb_synthesize_programme_mfcc: join is NULL"),
    "mfcc-programme-reserved": (-1, "jb_synthesize_programme_mfcc: reserved must be 0"),
    "mfcc-read": (-1, None),
    "mfcc-read_all": (-1, None),
    "mfcc-set": (-1, None),
    "mfcc-single-n_ceps": (-1, "jb_synthesize_batch_mfcc: " + N_CEPS),
    "mfcc-single-n_mels": (-1, "jb_synthesize_batch_mfcc: n_mels is in 1..128"),
    "mfcc-single-null": (-1, "jb_synthesize_batch_mfcc: the cepstral opts are NULL"),
    "mfcc-single-null_fbank": (-1, "jb_synthesize_batch_mfcc: opts is NULL"),
    "mfcc-single-null_outputs": (-1, None),
    "mfcc-size": (-1, None),
}


@pytest.mark.parametrize("case", sorted(EXPECTED))
def test_refusal(case):
    name, args = {**engine_cases(), **batch_cases()}[case]
    assert call(name, args) == EXPECTED[case], name


def test_every_case_is_recorded():
    assert sorted({**engine_cases(), **batch_cases()}) == sorted(EXPECTED)
    engine = {name for name, _ in engine_cases().values()}
    assert len(engine) == 23 and len(batch_cases()) == 21
