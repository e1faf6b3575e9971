"""The cases of the decode host-side table (tests/golden/decode_args.json) and how they are asked: shared by
tools/dev/record_decode_args.py, which records a library's answers, and tests/test_decode_args_host.py, which compares the
current library with the record.  Two kinds: the workspace queries of single-token attention (pure host functions that read no
pointer) and calls that the argument checks of the decode entry points refuse (status and wft_last_error text).  Every call here
is a refusal, on placeholder pointers and a null stream: nothing reaches a device, with or without a GPU."""
import ctypes

from whisper_finetune.engine import lib as L

PTR = 1 << 20  # placeholders with the alignment real operands have: nothing is dereferenced
ROWS = (1, 4, 5, 8, 30, 32, 40, 256, 257)
HEADS = (6, 20)
KEYS = (1, 448, 511, 512, 513, 1024, 1025, 1500, 8192, 8193)
GROUPS = (1, 3, 5, 8, 9)  # 9, a group that does not divide the rows and the self form with group != 1 answer 0
V, LD, EOT, TS_BEGIN, N_CTX = 51865, 51872, 50257, 50364, 448


def attn_args(rows, heads, tk, self_form, group=None):
    """A complete single-token attention call, packed operands: the beam struct, or with group=None the greedy one."""
    a = L.AttnDecodeArgs() if group is None else L.AttnDecodeBeamArgs()
    d = heads * 64
    a.q = a.k_cache = a.v_cache = a.o = PTR
    a.ldq = a.ldo = a.ld_cache = d
    a.cache_bs = tk * d
    a.H, a.Tk, a.scale = heads, tk, 0.125
    if group is None:
        a.B = rows
    else:
        a.R, a.group = rows, group
    if self_form:
        a.len = a.k_new = a.v_new = PTR
        a.ld_new = d
        if group is not None:
            a.anc, a.ld_anc = PTR, tk
    return a


def workspace_cases():
    """(rows, heads, Tk, self form, group or None for the greedy query) in table order."""
    return [(r, h, tk, form, g) for r in ROWS for h in HEADS for tk in KEYS for form in (False, True) for g in (None,) + GROUPS]


def workspace_bytes(h, case):
    a = attn_args(*case)
    query = h.wft_attn_decode_workspace_bytes if case[4] is None else h.wft_attn_decode_beam_workspace_bytes
    return int(query(ctypes.byref(a)))


def pick_args():
    a = L.DecodePickArgs()
    a.logits = a.first_len = a.tokens = a.len = a.finished = a.sum_logprob = a.unfinished = PTR
    a.ld, a.V, a.ld_tokens, a.B, a.eot, a.max_len = LD, V, N_CTX, 4, EOT, N_CTX
    return a


def topk_args():
    a = L.DecodeTopkArgs()
    a.logits = a.first_len = a.len = a.cand_tok = a.cand_logp = PTR
    a.ld, a.V, a.rows, a.row_step, a.k = LD, V, 4, 1, 6
    return a


def beam_args():
    a = L.BeamUpdateArgs()
    for name in ("cand_tok", "cand_logp", "tokens", "anc", "len", "sum_logprob", "done", "unfinished", "fin_tokens", "fin_len",
                 "fin_score", "fin_n"):
        setattr(a, name, PTR)
    a.ld_tokens = a.ld_anc = a.max_len = N_CTX
    a.B, a.W, a.C, a.eot = 2, 5, 5, EOT
    return a


def ts_rules():
    return L.TsRules(TS_BEGIN, TS_BEGIN - 1, 50)


def sample_rules():
    return L.SampleRules(PTR, PTR, 1)


# The edits that make a servable call refusable, one or more per WFT_CHECK_ARG line; {struct index: {field: value}}, None in place
# of the dict: that struct is passed as a null pointer.
ATTN_EDITS = [{"q": None}, {"o": None}, {"Tk": 0}, {"H": 0}, {"ldq": 320}, {"ld_cache": 376}, {"ldo": 388}, {"cache_bs": 448 * 384 + 4},
              {"cache_bs": 447 * 384 + 376}, {"k_cache": PTR + 8}, {"scale": 0.0}]
ATTN_SELF_EDITS = [{"k_new": None}, {"ld_new": 376}, {"ld_new": 388}, {"v_new": PTR + 8}]
ATTN_SPLIT_EDITS = [{}, {"workspace": PTR, "workspace_bytes": 3 * 6 * 66 * 4 - 4}, {"workspace": PTR + 8, "workspace_bytes": 1 << 20}]
PICK_EDITS = [{"logits": None}, {"unfinished": None}, {"B": 0}, {"V": 0x7ffffff1}, {"ld": LD - 8}, {"ld": LD + 4}, {"logits": PTR + 8},
              {"max_len": 0}, {"max_len": N_CTX + 1}, {"eot": -1}, {"eot": V}, {"suppress_first": PTR, "first_len": None}]
TS_EDITS = [{"ts_begin": EOT}, {"ts_begin": V}, {"no_timestamps": -2}, {"no_timestamps": V}]
SAMPLE_EDITS = [{"temperature": None}, {"seed": None}, {"group": 0}, {"group": 3}]
TOPK_EDITS = [{"cand_logp": None}, {"rows": 0}, {"row_step": 0}, {"k": 1}, {"k": 10}, {"ld": LD - 8}, {"logits": PTR + 2},
              {"suppress_first": PTR, "len": None}]
BEAM_EDITS = [{"anc": None}, {"unfinished": None}, {"fin_score": None}, {"B": 0}, {"W": 9}, {"C": 0}, {"max_len": N_CTX + 1},
              {"ld_anc": N_CTX - 1}, {"eot": -1}]
EMBED = (PTR, N_CTX, PTR, PTR, PTR, PTR, 4, N_CTX, 384, V)  # tokens, ld_tokens, len, emb, pos, out, B, n_ctx, d, V
EMBED_EDITS = [{0: None}, {5: None}, {6: 0}, {1: N_CTX - 1}, {8: 4}, {8: 388}, {9: 0}, {3: PTR + 8}]


def refusal_cases():
    """(entry point, [argument structs], {struct index: edits or None}, [plain arguments between the structs and the stream])"""
    out = []
    for entry, group in (("wft_attn_decode_bf16", None), ("wft_attn_decode_beam_bf16", 1)):
        out.append((entry, [attn_args(4, 6, 448, False, group)], {0: None}, []))
        out += [(entry, [attn_args(4, 6, 448, False, group)], {0: e}, []) for e in ATTN_EDITS]
        out += [(entry, [attn_args(4, 6, 448, True, group)], {0: e}, []) for e in ATTN_EDITS + ATTN_SELF_EDITS]
        out += [(entry, [attn_args(1, 6, 1500, form, group)], {0: e}, []) for form in (False, True) for e in ATTN_SPLIT_EDITS]
    beam = "wft_attn_decode_beam_bf16"
    out += [(beam, [attn_args(4, 6, 448, False, 1)], {0: {"group": g}}, []) for g in (0, 3, 9)]
    out += [(beam, [attn_args(4, 6, 448, True, 1)], {0: e}, []) for e in ({"group": 2}, {"anc": None}, {"ld_anc": 447})]
    for entry, rules in (("wft_decode_pick", []), ("wft_decode_pick_ts", [ts_rules]), ("wft_decode_sample", [sample_rules]),
                         ("wft_decode_sample_ts", [sample_rules, ts_rules])):
        make = lambda rules=rules: [pick_args()] + [r() for r in rules]  # noqa: E731
        out.append((entry, make(), {0: None}, []))
        out += [(entry, make(), {0: e}, []) for e in PICK_EDITS]
        for i, r in enumerate(rules, 1):
            out.append((entry, make(), {i: None}, []))
            out += [(entry, make(), {i: e}, []) for e in (TS_EDITS if r is ts_rules else SAMPLE_EDITS)]
        if ts_rules in rules:
            out.append((entry, make(), {0: {"first_len": None}}, []))
    out.append(("wft_decode_sample_ts", [pick_args(), sample_rules(), ts_rules()], {1: {"group": 0}, 2: None}, []))  # the order of the checks
    for entry, extra in (("wft_decode_topk", None), ("wft_decode_topk_ts", [PTR, N_CTX, EOT])):
        make = lambda extra=extra: [topk_args()] + ([ts_rules()] if extra else [])  # noqa: E731
        out.append((entry, make(), {0: None}, extra or []))
        out += [(entry, make(), {0: e}, extra or []) for e in TOPK_EDITS]
    ts = "wft_decode_topk_ts"
    out += [(ts, [topk_args(), ts_rules()], {}, [PTR, N_CTX, eot]) for eot in (-1, V)]
    out.append((ts, [topk_args(), ts_rules()], {1: None}, [PTR, N_CTX, EOT]))
    out += [(ts, [topk_args(), ts_rules()], {1: e}, [PTR, N_CTX, EOT]) for e in TS_EDITS]
    out += [(ts, [topk_args(), ts_rules()], {0: {f: None}}, [PTR, N_CTX, EOT]) for f in ("first_len", "len")]
    out += [(ts, [topk_args(), ts_rules()], {}, extra) for extra in ([None, N_CTX, EOT], [PTR, 0, EOT])]
    out.append(("wft_beam_update", [beam_args()], {0: None}, []))
    out += [("wft_beam_update", [beam_args()], {0: e}, []) for e in BEAM_EDITS]
    for edit in EMBED_EDITS:
        args = list(EMBED)
        for i, v in edit.items():
            args[i] = v
        out.append(("wft_decode_embed", [], {}, args))
    return out


def refusal(h, case):
    """[status, wft_last_error text] of one case"""
    entry, structs, edits, plain = case
    refs = []
    for i, s in enumerate(structs):
        e = edits.get(i, {})
        for field, value in (e or {}).items():
            setattr(s, field, value)
        refs.append(None if e is None else ctypes.byref(s))
    rc = getattr(h, entry)(*refs, *plain, None)
    return [int(rc), h.wft_last_error().decode()]


def all_answers(h):
    return {"workspace": [workspace_bytes(h, c) for c in workspace_cases()], "refusals": [refusal(h, c) for c in refusal_cases()]}
