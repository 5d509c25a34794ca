"""Decoding for FlamingoModel.generate(): the option tuples, the routing rule, the fixed-shape sessions (one class per strategy) and the
dynamic loops.  Nothing here knows the model classes: a session reads `model.flamingo` (its `lm_family`, its LM config, its forward), the
dynamic loops take the model's `_decode_step` / `_reorder_cache` as callables.  modeling_flamingo.py keeps thin methods that delegate here.
"""
from __future__ import annotations

import dataclasses
import weakref
from typing import NamedTuple, Optional

import torch

from . import functional as F
from .graphs import _prepared_capture_stream


# ---- options: NamedTuples, so they compare and hash equal to the plain tuples they replaced (session keys, tests, tools) ----
Sampling = NamedTuple("Sampling", [("temperature", float), ("top_k", int), ("top_p", float)])
Beams = NamedTuple("Beams", [("nb", int), ("early_stopping", bool), ("length_penalty", float)])
Groups = NamedTuple("Groups", [("n", int), ("diversity_penalty", float)])      # diverse beam search: beside Beams, which keeps its three fields
# the truncation samplers: beside Sampling, which keeps its three fields
Truncation = NamedTuple("Truncation", [("min_p", float), ("typical_p", float), ("epsilon_cutoff", float), ("eta_cutoff", float)])
# contrastive search: k candidates per sequence and step (a session's shape: part of its key), alpha (a device scalar of the session: not part of it)
Contrastive = NamedTuple("Contrastive", [("k", int), ("penalty_alpha", float)])


class Processors(NamedTuple):
    repetition_penalty: float
    no_repeat_ngram_size: int
    min_length: int
    min_new_tokens: int

    def min_len(self, L0: int) -> int:
        """The length below which eos is banned, for a prompt of L0 tokens."""
        return max(self.min_length, L0 + self.min_new_tokens)

    def given(self):
        """The names of the arguments that are not at their off value."""
        return [n for n, v, off in zip(self._fields, self, (1, 0, 0, 0)) if v != off]


@dataclasses.dataclass
class GenerateOutput:
    """What generate(return_dict_in_generate=True) returns.  `sequences` (rows, width) are the ids generate() returns without the flag.
    `token_logprobs` (rows, width - L0), greedy and sampling with output_logprobs=True: the log-softmax, at the chosen token, of the step's
    logits as the selection sees them (after the logits processors, before temperature / top-k / top-p); 0 at the pad positions of a row
    that had finished, the eos token carries its own.  `sequences_scores` (rows,): beam search - the normalised score the search ranked by;
    greedy and sampling with output_logprobs=True - sum(token_logprobs) / float32(len ** length_penalty), len = the prompt's length plus
    the generated tokens up to and including eos.  A field that was not computed is None."""
    sequences: torch.Tensor
    sequences_scores: Optional[torch.Tensor] = None
    token_logprobs: Optional[torch.Tensor] = None


def _repeat_leading(t: torch.Tensor, m: int) -> torch.Tensor:
    """'n ... -> (n m) ...' (each row repeated m times, as beam search does with input_ids)."""
    return t.repeat_interleave(m, dim=0)


# ---- generate(): argument checks and the static / dynamic decision ----
def check_generate_args(unsupported, use_cache, repetition_penalty, no_repeat_ngram_size, min_length, min_new_tokens, eos) -> Optional[Processors]:
    """The argument checks of generate(), in its order.  Returns the logits processors, None when every one is off (exactly the paths
    without them)."""
    if unsupported:
        raise TypeError(f"generate(): unsupported generation arguments {sorted(unsupported)}")
    if not use_cache:
        raise ValueError("generate() always decodes with the cross-attention / LM caches (use_cache=True)")
    if isinstance(repetition_penalty, bool) or not isinstance(repetition_penalty, (int, float)) or not 0 < repetition_penalty < float("inf"):
        raise ValueError(f"generate(): repetition_penalty must be a positive, finite number (1 = off), got {repetition_penalty!r}")
    for name, v in (("no_repeat_ngram_size", no_repeat_ngram_size), ("min_length", min_length), ("min_new_tokens", min_new_tokens)):
        if isinstance(v, bool) or not isinstance(v, int) or v < 0:
            raise ValueError(f"generate(): {name} must be an integer >= 0 (0 = off), got {v!r}")
    if (min_length > 0 or min_new_tokens > 0) and eos is None:
        raise ValueError("generate(): min_length / min_new_tokens need eos_token_id")
    procs = Processors(float(repetition_penalty), int(no_repeat_ngram_size), int(min_length), int(min_new_tokens))
    return procs if procs.given() else None


# ---- constrained decoding: the host-built tables of ff_logits_constrain (include/flamingo_fusion.h) ----
CONSTRAINT_TABLE_MAX = 1 << 22         # entries per table a session will hold on the device (16 MiB of int32); larger sets take the dynamic loop
_TABLE_FLOORS = (64, 64, 16, 64)       # node_cap, edge_cap, bw_cap, bw_tok_cap: the smallest capacities a session allocates


def _id_lists(name, lists, vocab):
    """`lists` as a sorted list of distinct tuples of ints in [0, vocab); ValueError for anything else, empty input and empty entries."""
    if isinstance(lists, (str, bytes)) or not hasattr(lists, "__iter__"):
        raise ValueError(f"generate(): {name} must be a list of lists of token ids, got {lists!r}")
    out = set()
    for entry in lists:
        if isinstance(entry, (str, bytes)) or not hasattr(entry, "__iter__"):
            raise ValueError(f"generate(): {name} must be a list of lists of token ids, got the entry {entry!r}")
        entry = tuple(entry)
        if not entry:
            raise ValueError(f"generate(): {name} holds an empty entry")
        for t in entry:
            if isinstance(t, bool) or not isinstance(t, int) or not 0 <= t < vocab:
                raise ValueError(f"generate(): {name} holds {t!r}, not a token id in [0, {vocab})")
        out.add(entry)
    if not out:
        raise ValueError(f"generate(): {name} is empty")
    return sorted(out)


def _cap(n, floor):
    """n rounded up to a power of two, at least `floor`: the capacity class of a table of n entries."""
    return max(floor, 1 << max(int(n) - 1, 0).bit_length())


class TokenTrie:
    """The candidate sequences of generate(candidate_ids=...) as the CSR trie ff_logits_constrain reads: root = node 0, the edges of node s
    are node_first[s] .. node_first[s + 1], edge_tok ascending inside a node, node_terminal[s] = a candidate ends at s.  Duplicates are
    dropped; a candidate that is a prefix of another makes an inner node terminal (there eos and the longer candidate's next token are both
    allowed).  ValueError: no candidates, an empty candidate, an id outside [0, vocab), a candidate that contains eos."""

    def __init__(self, candidates, vocab, eos):
        import numpy as np
        cands = _id_lists("candidate_ids", candidates, vocab)
        if any(eos in c for c in cands):
            raise ValueError(f"generate(): a candidate contains eos_token_id {eos}; eos ends a candidate, it cannot be part of one")
        children, terminal = [{}], [False]
        for c in cands:
            s = 0
            for t in c:
                nxt = children[s].get(t)
                if nxt is None:
                    nxt = children[s][t] = len(children)
                    children.append({})
                    terminal.append(False)
                s = nxt
            terminal[s] = True
        self.vocab, self.candidates, self.longest = vocab, cands, max(len(c) for c in cands)
        self.n_nodes = len(children)
        self.node_first = np.cumsum([0] + [len(ch) for ch in children]).astype(np.int32)
        self.edge_tok = np.array([t for ch in children for t in sorted(ch)], np.int32)
        self.edge_child = np.array([ch[t] for ch in children for t in sorted(ch)], np.int32)
        self.node_terminal = np.array(terminal, np.uint8)

    DEAD, DONE = -1, -2

    def walk(self, generated, eos):
        """Rule T1: the node the generated tokens lead to, or DONE / DEAD."""
        import numpy as np
        s = 0
        for t in generated:
            if t == eos and self.node_terminal[s]:
                return self.DONE
            lo, hi = int(self.node_first[s]), int(self.node_first[s + 1])
            i = lo + int(np.searchsorted(self.edge_tok[lo:hi], t))
            if i == hi or int(self.edge_tok[i]) != t:
                return self.DEAD
            s = int(self.edge_child[i])
        return s

    def allowed(self, s, eos):
        """Rule T2: the tokens node s allows."""
        toks = self.edge_tok[int(self.node_first[s]):int(self.node_first[s + 1])].tolist()
        return toks + [eos] if self.node_terminal[s] else toks


class BadWords:
    """The words of generate(bad_words_ids=...) as the table ff_logits_constrain reads: word w is bw_tok[bw_off[w] .. bw_off[w + 1]).
    Duplicates are dropped.  ValueError: no words, an empty word, an id outside [0, vocab)."""

    def __init__(self, words, vocab):
        import numpy as np
        self.words = _id_lists("bad_words_ids", words, vocab)
        self.vocab, self.n = vocab, len(self.words)
        self.bw_off = np.cumsum([0] + [len(w) for w in self.words]).astype(np.int32)
        self.bw_tok = np.array([t for w in self.words for t in w], np.int32)


class Constraints:
    """What generate(candidate_ids=, bad_words_ids=) decodes under: a TokenTrie and / or BadWords (either may be None, not both)."""

    def __init__(self, trie=None, bad_words=None):
        assert trie is not None or bad_words is not None
        self.trie, self.bad_words = trie, bad_words

    def caps(self):
        """("constraints", node_cap, edge_cap, bw_cap, bw_tok_cap): the capacity class of the tables - the live sizes rounded up to powers of
        two, 0 for an absent table - and the trailing element of the key of a session that decodes under them: calls whose tables fall into
        the same class share the session and its captured graph."""
        t, w = self.trie, self.bad_words
        sizes = (t.n_nodes, len(t.edge_tok)) if t is not None else (None, None)
        sizes += (w.n, len(w.bw_tok)) if w is not None else (None, None)
        return ("constraints",) + tuple(0 if n is None else _cap(n, f) for n, f in zip(sizes, _TABLE_FLOORS))


def check_constraint_args(candidate_ids, bad_words_ids, vocab, eos, procs, L0, max_length) -> Optional[Constraints]:
    """The checks of generate()'s constraint arguments.  Returns the Constraints, None when both are None (exactly the paths without them)."""
    if candidate_ids is None and bad_words_ids is None:
        return None
    trie = None
    if candidate_ids is not None:
        if eos is None:
            raise ValueError("generate(): candidate_ids needs eos_token_id (eos is what ends a candidate)")
        if procs is not None and (procs.min_length > 0 or procs.min_new_tokens > 0):
            raise ValueError("generate(): candidate_ids cannot be combined with min_length / min_new_tokens: at the end of a candidate only eos is "
                             "allowed, and while the minimum length bans eos no token would be")
        trie = TokenTrie(candidate_ids, vocab, eos)
        if L0 + trie.longest + 1 > max_length:
            raise ValueError(f"generate(): the prompt ({L0} tokens), the longest candidate ({trie.longest}) and eos do not fit max_length {max_length}")
    return Constraints(trie, BadWords(bad_words_ids, vocab) if bad_words_ids is not None else None)


def check_output_args(return_dict_in_generate, output_logprobs, num_return_sequences, num_beams, do_sample) -> int:
    """The checks of generate()'s output arguments.  Returns num_return_sequences."""
    n = num_return_sequences
    if isinstance(n, bool) or not isinstance(n, int) or n < 1:
        raise ValueError(f"generate(): num_return_sequences must be an integer >= 1, got {n!r}")
    if output_logprobs and not return_dict_in_generate:
        raise ValueError("generate(): output_logprobs=True needs return_dict_in_generate=True")
    if output_logprobs and num_beams > 1:
        raise ValueError("generate(): output_logprobs=True is not offered with beam search (per-token values would be differences of rounded "
                         "running sums); sequences_scores holds the score the search ranked by")
    if n > 1 and num_beams > 1 and n > num_beams:
        raise ValueError(f"generate(): num_return_sequences {n} exceeds num_beams {num_beams}")
    if n > 1 and num_beams <= 1 and not do_sample:
        raise ValueError("generate(): num_return_sequences > 1 needs do_sample=True or num_beams > 1 (greedy decoding has one result)")
    return n


def check_group_args(num_beam_groups, diversity_penalty, num_beams, do_sample) -> Optional[Groups]:
    """The checks of generate()'s diverse-beam-search arguments.  Returns the Groups, None for one group (exactly the paths without them)."""
    G, lam = num_beam_groups, diversity_penalty
    if isinstance(G, bool) or not isinstance(G, int) or G < 1:
        raise ValueError(f"generate(): num_beam_groups must be an integer >= 1, got {G!r}")
    if isinstance(lam, bool) or not isinstance(lam, (int, float)) or not 0 <= lam < float("inf"):
        raise ValueError(f"generate(): diversity_penalty must be a finite number >= 0 (0 = off), got {lam!r}")
    if num_beams % G != 0:
        raise ValueError(f"generate(): num_beams {num_beams} is not a multiple of num_beam_groups {G}")
    if G > 1 and do_sample:
        raise ValueError("generate(): num_beam_groups > 1 cannot be combined with do_sample")
    if G == 1 and lam != 0:
        raise ValueError("generate(): diversity_penalty needs num_beam_groups > 1 (one group has nobody to differ from)")
    return Groups(G, float(lam)) if G > 1 else None


def check_guidance_args(guidance_scale) -> Optional[float]:
    """The check of generate()'s guidance_scale.  Returns the scale as a float, None for 1.0 (off: exactly the paths without it)."""
    g = guidance_scale
    if isinstance(g, bool) or not isinstance(g, (int, float)) or not 0 <= g < float("inf"):
        raise ValueError(f"generate(): guidance_scale must be a finite number >= 0 (1 = off), got {g!r}")
    return float(g) if g != 1 else None


def check_truncation_args(min_p, typical_p, epsilon_cutoff, eta_cutoff, do_sample, num_beams) -> Optional[Truncation]:
    """The checks of generate()'s truncation samplers.  Returns the Truncation, None when all four are off (exactly the paths without them)."""
    num = lambda v: not isinstance(v, bool) and isinstance(v, (int, float))
    if not (num(min_p) and 0 <= min_p <= 1):
        raise ValueError(f"generate(): min_p must be a number in [0, 1] (0 = off), got {min_p!r}")
    if not (num(typical_p) and 0 < typical_p <= 1):
        raise ValueError(f"generate(): typical_p must be a number in (0, 1] (1 = off), got {typical_p!r}")
    for name, v in (("epsilon_cutoff", epsilon_cutoff), ("eta_cutoff", eta_cutoff)):
        if not (num(v) and 0 <= v < 1):
            raise ValueError(f"generate(): {name} must be a number in [0, 1) (0 = off), got {v!r}")
    t = Truncation(float(min_p), float(typical_p), float(epsilon_cutoff), float(eta_cutoff))
    if t == (0.0, 1.0, 0.0, 0.0):
        return None
    given = [n for n, v, off in zip(t._fields, t, (0.0, 1.0, 0.0, 0.0)) if v != off]
    if num_beams > 1:
        raise ValueError(f"generate(): {given} are not offered with beam search (num_beams > 1)")
    if not do_sample:
        raise ValueError(f"generate(): {given} need do_sample=True (they truncate the distribution a token is sampled from)")
    return t


def check_contrastive_args(penalty_alpha, top_k, do_sample, num_beams, num_beam_groups=1, guidance_scale=1.0, num_return_sequences=1) -> Optional[Contrastive]:
    """The checks of generate()'s penalty_alpha.  Returns the Contrastive, None for 0 (off: exactly the paths without it, top_k stays what it
    was to them).  On for 0 < penalty_alpha <= 1 together with 2 <= top_k <= 8, do_sample=False, num_beams == 1, one beam group, no guidance
    and one returned sequence; everything else raises ValueError."""
    a = penalty_alpha
    if isinstance(a, bool) or not isinstance(a, (int, float)) or not 0 <= a <= 1:             # (NaN fails both comparisons)
        raise ValueError(f"generate(): penalty_alpha must be a number in [0, 1] (0 = off), got {a!r}")
    if a == 0:
        return None
    if isinstance(top_k, bool) or not isinstance(top_k, int) or not 2 <= top_k <= F.ffi.CONTRASTIVE_K_MAX:
        raise ValueError(f"generate(): contrastive search (penalty_alpha > 0) needs an integer top_k in [2, {F.ffi.CONTRASTIVE_K_MAX}], got {top_k!r}")
    if do_sample:
        raise ValueError("generate(): penalty_alpha cannot be combined with do_sample (contrastive search is deterministic)")
    if num_beams > 1 or num_beam_groups > 1:
        raise ValueError("generate(): penalty_alpha cannot be combined with beam search (num_beams > 1, num_beam_groups > 1)")
    if guidance_scale != 1:
        raise ValueError("generate(): penalty_alpha cannot be combined with guidance_scale")
    if num_return_sequences > 1:
        raise ValueError("generate(): penalty_alpha cannot be combined with num_return_sequences > 1 (contrastive search has one result)")
    return Contrastive(int(top_k), float(a))


def sequence_scores(sequences, token_logprobs, L0, eos, length_penalty):
    """sum(token_logprobs) / float32(len ** length_penalty) per row, len = L0 + the generated tokens up to and including eos: beam search's
    normalisation (BeamState.len_norm) applied to greedy and sampled sequences."""
    gen = sequences[:, L0:]
    n_gen = torch.full((gen.shape[0],), gen.shape[1], dtype=torch.long, device=gen.device)
    if eos is not None and gen.shape[1] > 0:
        hit = gen == eos
        n_gen = torch.where(hit.any(1), hit.long().argmax(1) + 1, n_gen)
    norm = torch.tensor([float(L0 + int(k)) ** length_penalty for k in n_gen.tolist()], dtype=torch.float32, device=gen.device)
    return token_logprobs.sum(1) / norm.to(token_logprobs.dtype)


def route(*, is_cuda, num_beams, do_sample, static_decode, model_default, lm_family, L0, max_length, ids_is_int64, procs_on, procs_given=(),
          logprobs_on=False, constraints_on=False, vocab=0, table_entries=0, guidance_on=False, beam_sample_on=False, contrastive_on=False):
    """Which path a generate() call takes: "static" (a _DecodeSession) or "dynamic" (dynamic_decode / beam_search), from plain values only.
    `static_decode` is generate()'s argument (None, True, False), `model_default` the model's attribute, `procs_given` the processor
    arguments' names for the TypeError on CPU tensors.  Greedy decoding takes the static path by default on the GPU; sampling and beam search
    only when static_decode=True is passed, and then they need GPU tensors: their kernels have no CPU form.  Neither has the log-probability
    kernel (`logprobs_on`): a static session that records them needs GPU tensors, CPU tensors take the dynamic loop unless static_decode=True
    asks for what cannot be had.  Constraints (`constraints_on`, with the LM's `vocab` and `table_entries`, the largest table's size) are
    the same on CPU tensors - the dynamic loops restate them on the host - and take the static path under the processors' conditions
    plus the kernel's vocabulary cap and the sessions' table cap.  Guidance (`guidance_on`) routes like the log-probabilities: its kernel has
    no CPU form but its torch restatement has one, so CPU tensors take the dynamic loop unless static_decode=True asks for what cannot be
    had; guided greedy decoding is static by default on the GPU, guided sampling and beam search on request.
    `do_sample` here means TOKEN sampling (one token per row from its own distribution): together with num_beams > 1 it raises, as it always
    has.  Beam sampling (generate(num_beams > 1, do_sample=True)) is a beam search whose selection draws: generate() asks for it with
    do_sample=False and `beam_sample_on=True`, and it routes exactly like beam search - static only with static_decode=True, which on CPU
    tensors raises what ffi.require_cuda raises (its kernel has no CPU form), otherwise the dynamic loop, which also runs on CPU tensors.
    Contrastive search (`contrastive_on`, with num_beams = 1 and do_sample=False) routes like beam search too: a _ContrastiveSession only
    with static_decode=True, which needs GPU tensors; otherwise decoding.contrastive_search, which also runs on CPU tensors."""
    def need_gpu():                     # what ffi.require_cuda raises for a CPU tensor
        if not is_cuda:
            F.ffi.require_cuda(torch.empty(0))

    if procs_on and not is_cuda:        # GPU tensors only: on CPU tensors the processors stay what they were, unsupported
        if static_decode:
            need_gpu()
        raise TypeError(f"generate(): unsupported generation arguments {list(procs_given)} on CPU tensors (the logits processors run on the GPU only)")
    if num_beams > 1 and do_sample:
        raise ValueError("beam search with sampling is not implemented")
    on_request = num_beams > 1 or do_sample or beam_sample_on or contrastive_on                 # static only when static_decode=True is passed
    if (on_request or logprobs_on or constraints_on or guidance_on) and static_decode:
        need_gpu()
    if static_decode is None:
        static_decode = is_cuda and model_default and not on_request
    static_ok = lm_family is not None and L0 + 1 < max_length and num_beams <= F.ffi.BEAM_MAX and (not (procs_on or constraints_on) or (ids_is_int64 and max_length <= F.ffi.LOGITS_HIST_MAX)) and \
        (not constraints_on or (vocab <= F.ffi.CONSTRAIN_VOCAB_MAX and table_entries <= CONSTRAINT_TABLE_MAX))
    return "static" if static_decode and static_ok else "dynamic"


# ---- logits rules of the dynamic loops, in torch (FlamingoModel._filter_logits / ._process_logits) ----
def filter_logits(logits, temperature, top_k, top_p):
    """temperature / top-k / nucleus filtering as in transformers' logits warpers."""
    if temperature != 1.0:
        logits = logits / temperature
    if top_k and top_k > 0:
        kth = logits.topk(min(top_k, logits.shape[-1]), dim=-1).values[..., -1, None]
        logits = logits.masked_fill(logits < kth, float("-inf"))
    if top_p < 1.0:
        srt, idx = logits.sort(dim=-1, descending=True)
        cum = srt.softmax(-1).cumsum(-1)
        drop = cum - srt.softmax(-1) >= top_p               # keep the smallest prefix whose mass reaches top_p
        logits = logits.masked_fill(drop.scatter(-1, idx, drop), float("-inf"))
    return logits


def truncate_logits_torch(logits, min_p=0.0, typical_p=1.0, epsilon_cutoff=0.0, eta_cutoff=0.0):
    """Rules 3 - 6 of ff_sample_token_truncated (include/flamingo_fusion.h) in torch, on tensors of any device and in their own dtype: min_p,
    typical_p, epsilon_cutoff and eta_cutoff as transformers' MinPLogitsWarper, TypicalLogitsWarper, EpsilonLogitsWarper and EtaLogitsWarper
    (min_tokens_to_keep = 1) apply them, in that order.  `logits` (rows, V) are what filter_logits returns: divided by the temperature, -inf
    where top-k / top-p dropped a column.  Every stage drops by value - equal values stay or go together - and keeps the columns of the
    largest value it was given.  Returns new logits, dropped columns -inf."""
    ninf = float("-inf")
    top = lambda x: x.amax(-1, keepdim=True)
    entropy = lambda lp: -torch.where(lp > ninf, lp.exp() * lp, torch.zeros_like(lp)).sum(-1, keepdim=True)
    if min_p > 0:
        logits = logits.masked_fill((logits - top(logits)).exp() < min_p, ninf)
    if typical_p < 1:
        lp = logits.log_softmax(-1)
        d, idx = (-lp - entropy(lp)).abs().sort(-1)                        # ascending; the -inf columns have d = inf and come last
        r = lp.exp().gather(-1, idx)
        before = r.cumsum(-1) - r                                          # the mass sorted in front of a column ...
        first = torch.ones_like(d, dtype=torch.bool)
        first[..., 1:] = d[..., 1:] != d[..., :-1]
        before = torch.where(first, before, torch.zeros_like(before)).cummax(-1).values      # ... of STRICTLY smaller d: that of its run's first
        drop = before >= typical_p
        logits = logits.masked_fill(drop.scatter(-1, idx, drop), ninf)
    if epsilon_cutoff > 0:
        logits = logits.masked_fill((logits.softmax(-1) < epsilon_cutoff) & (logits < top(logits)), ninf)
    if eta_cutoff > 0:
        lp = logits.log_softmax(-1)
        eta = torch.clamp(eta_cutoff ** 0.5 * (-entropy(lp)).exp(), max=eta_cutoff)
        logits = logits.masked_fill((lp.exp() < eta) & (logits < top(logits)), ninf)
    return logits


def gumbel_noise_torch(shape, generator=None, device=None):
    """Standard Gumbel noise as rule S4 of ff_beam_sample_step forms it from a uniform number: u on the 23-bit grid ((k + 0.5) 2^-23, k <
    2^23: strictly inside (0, 1)), g = -log(-log(u)) - with the uniform numbers from torch.rand(generator=), not from the kernel's Philox."""
    u = (torch.rand(shape, generator=generator, device=device, dtype=torch.float32) * 2.0 ** 23).floor().add_(0.5).mul_(2.0 ** -23)
    return -(-u.log()).log()


def beam_sample_select_torch(logits, score, g, nb, temperature=1.0, top_k=0, top_p=1.0):
    """Rules S1 - S5 of ff_beam_sample_step (include/flamingo_fusion.h) in torch, on tensors of any device: `logits` (b * nb, V), `score`
    (b, nb) the beams' running scores, `g` (b * nb, V) the noise.  Per row: lse and logp = x - lse; top-k by value (ties kept) and the nucleus
    over softmax(logp / T) within it (equal values stay or go together, the maximum stays); z = logp / T where kept, -inf elsewhere, nothing
    renormalised; a = z + score; p = a + g.  Per sequence the 2 nb largest p, by p descending, then flat index ascending - a Gumbel top-k: a
    draw of 2 nb continuations without replacement from softmax(a).  The math is float32, float64 for float64 logits.
    Returns (a, beam, token), each (b, 2 nb), in the order of p."""
    dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    x = logits.to(dt)
    rows, V = x.shape
    b, ninf = rows // nb, float("-inf")
    m = x.amax(-1, keepdim=True)
    logp = x - (m + (x - m).exp().sum(-1, keepdim=True).log())
    keep = torch.ones_like(x, dtype=torch.bool)
    if 0 < top_k < V:
        keep = x >= x.topk(top_k, dim=-1).values[..., -1:]
    if top_p < 1.0:
        keep = keep & (x > ninf)
        srt, idx = x.masked_fill(~keep, ninf).sort(-1, descending=True)
        w = torch.where(srt > ninf, ((srt - m) * (1.0 / temperature)).exp(), torch.zeros_like(srt))
        before = w.cumsum(-1) - w                                           # the mass sorted in front of a column ...
        first = torch.ones_like(keep)
        first[..., 1:] = srt[..., 1:] != srt[..., :-1]
        above = torch.where(first, before, torch.zeros_like(before)).cummax(-1).values      # ... of STRICTLY larger values: that of its run's first
        drop = above >= top_p * w.sum(-1, keepdim=True)
        keep = keep & ~torch.zeros_like(keep).scatter(-1, idx, drop)
    z = logp if temperature == 1.0 else logp / temperature
    a = (torch.where(keep, z, torch.full_like(z, ninf)) + score.to(dt).reshape(-1, 1)).reshape(b, nb * V)
    p = a + g.to(dt).reshape(b, nb * V)
    flat = p.sort(dim=-1, descending=True, stable=True).indices[:, :2 * nb]    # (a stable sort: the lower flat index on equal p)
    return a.gather(-1, flat), flat // V, flat % V


def order_by_score(a, beam, token, V):
    """Rule S6: the drawn candidates ordered by accumulated score descending, then flat index ascending.  Returns (a, flat index)."""
    flat = beam * V + token
    o = flat.argsort(dim=-1, stable=True)
    a, flat = a.gather(-1, o), flat.gather(-1, o)
    o = a.argsort(dim=-1, descending=True, stable=True)
    return a.gather(-1, o), flat.gather(-1, o)


def topk_logprobs_torch(logits, k):
    """Rule T of contrastive search (include/flamingo_fusion.h) in torch, on tensors of any device: per row of `logits` (rows, V) the k
    largest values, by value descending, then by index ascending, with logp = x - lse (lse = max + log(sum exp(x - max))); a -inf logit is
    listed only when fewer than k finite ones exist and carries logp = -inf.  The math is float32, float64 for float64 logits.
    Returns (tok (rows, k) int64, logp (rows, k))."""
    dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    x = logits.to(dt)
    m = x.amax(-1, keepdim=True)
    lse = m + (x - m).exp().sum(-1, keepdim=True).log()
    val, tok = x.sort(dim=-1, descending=True, stable=True)                 # (a stable sort: the lower index on equal values)
    val, tok = val[:, :k], tok[:, :k]
    return tok, torch.where(val > float("-inf"), val - lse, torch.full_like(val, float("-inf")))


def contrastive_select_torch(hidden, hist, mask, cand_tok, cand_logp, finished, alpha, eos=None, pad=0):
    """Rules C2 - C6 of contrastive search (include/flamingo_fusion.h) in torch, on tensors of any device: `hidden` (b * k, dim) the
    candidates' lm_head inputs, `hist` (b, n, dim) those of the n positions so far, `mask` (b, n) - 0 excludes a position -, `cand_tok` /
    `cand_logp` (b, k), `finished` (b,) bool (not modified).  cos = <h_c, H_j> / (max(|h_c|, 1e-12) max(|H_j|, 1e-12)), pen = the maximum
    over the live positions (0 without one), score = (1 - alpha) exp(logp) - alpha pen, -inf for a dead candidate (logp = -inf); c* = the
    smallest c of maximal score.  The math is float32, float64 for float64 `hidden`.
    Returns (next_tok (b,), logprob (b,), c* (b,), finished after the step (b,), score (b, k))."""
    dt = torch.float64 if hidden.dtype == torch.float64 else torch.float32
    b, k = cand_tok.shape
    h = hidden.to(dt).reshape(b, k, -1)
    H = hist.to(dt)
    hn = h.square().sum(-1).sqrt().clamp(min=1e-12)                            # (b, k)
    Hn = H.square().sum(-1).sqrt().clamp(min=1e-12)                            # (b, n)
    cos = torch.einsum("bkd,bnd->bkn", h, H) / (hn[:, :, None] * Hn[:, None, :])
    live = (mask != 0)[:, None, :].expand(b, k, -1)
    if live.shape[-1] > 0:
        pen = cos.masked_fill(~live, float("-inf")).amax(-1)
        pen = torch.where(pen > float("-inf"), pen, torch.zeros_like(pen))
    else:
        pen = torch.zeros((b, k), dtype=dt, device=hidden.device)
    lp = cand_logp.to(dt)
    score = torch.where(lp > float("-inf"), (1.0 - alpha) * lp.exp() - alpha * pen, torch.full_like(lp, float("-inf")))
    best = score.amax(-1, keepdim=True)
    first = (score == best) & (best > float("-inf"))                          # every candidate dead: no True, and c* = k % k = 0
    c = torch.where(first, torch.arange(k, device=score.device).expand(b, k), torch.full((b, k), k, device=score.device)).amin(-1) % k
    tok = cand_tok.gather(1, c[:, None])[:, 0]
    logprob = lp.gather(1, c[:, None])[:, 0]
    nxt = torch.where(finished, torch.full_like(tok, pad), tok)
    logprob = torch.where(finished, torch.zeros_like(logprob), logprob)
    done = finished | (nxt == eos) if eos is not None else finished.clone()
    return nxt, logprob, c, done, score


def process_logits(logits, seqs, repetition_penalty, no_repeat_ngram_size, eos, min_len):
    """Repetition penalty, no-repeat n-gram ban and minimum length on float32 `logits` (rows, V) against the sequences so far `seqs`
    (rows, n): the rules of ff_logits_process (include/flamingo_fusion.h) restated in torch for the dynamic loops, with the same
    x * (1.0f / p) where transformers divides.  Returns new logits."""
    V, n = logits.shape[-1], seqs.shape[1]
    seqs = seqs.long()
    valid = (seqs >= 0) & (seqs < V)
    out = torch.cat([logits, logits.new_zeros(logits.shape[0], 1)], dim=1)          # column V takes what out-of-range ids would write
    if repetition_penalty != 1.0 and n > 0:
        import numpy as np
        p = np.float32(repetition_penalty)
        idx = torch.where(valid, seqs, torch.full_like(seqs, V))
        x = out.gather(1, idx)
        out.scatter_(1, idx, torch.where(x < 0, x * float(p), x * float(np.float32(1.0) / p)))
    if 1 <= no_repeat_ngram_size <= n:
        g = no_repeat_ngram_size
        win = seqs.unfold(1, g, 1)                                                   # (rows, n - g + 1, g)
        match = (win[..., :g - 1] == seqs[:, None, n - g + 1:]).all(-1)
        out.scatter_(1, torch.where(match & valid[:, g - 1:], win[..., -1], torch.full_like(win[..., -1], V)), float("-inf"))
    if eos is not None and min_len is not None and n < min_len:
        out[:, eos] = float("-inf")
    return out[:, :V].contiguous()


def constrain_logits_torch(logits, seqs, gen_start, eos, trie=None, bad_words=None):
    """The rules of ff_logits_constrain (T1, T2, B1 of include/flamingo_fusion.h) for the dynamic loops, on tensors of any device: `logits`
    (rows, V) against the sequences so far `seqs` (rows, n), whose generated tokens begin at `gen_start`; `trie` a TokenTrie, `bad_words` a
    BadWords.  The trie is walked on the host (one read of `seqs`), the bans are one masked_fill.  Returns new logits."""
    V, n = logits.shape[-1], seqs.shape[1]
    n0 = min(max(int(gen_start), 0), n)
    ban = torch.zeros(logits.shape, dtype=torch.bool)
    for r, h in enumerate(seqs.tolist()):
        if trie is not None:
            s = trie.walk(h[n0:], eos)
            if s >= 0:                                                            # DONE and DEAD rows stay untouched
                ban[r] = True
                ban[r, [t for t in trie.allowed(s, eos) if 0 <= t < V]] = False
        for w in (bad_words.words if bad_words is not None else ()):
            m = len(w)
            if 0 <= w[-1] < V and n >= m - 1 and tuple(h[n - m + 1:]) == w[:-1]:
                ban[r, w[-1]] = True
    return logits.masked_fill(ban.to(logits.device), float("-inf"))


def guided_logits_torch(cond, uncond, scale):
    """The rules of ff_guided_logits (G1 - G3 of include/flamingo_fusion.h) in torch, for the dynamic loops and for CPU tensors: lu + scale *
    (lc - lu) with lc / lu the log-softmax of `cond` / `uncond` (rows, V), in float32 - in float64 for float64 inputs.  An entry that is
    -inf in either input is -inf for every scale; a row pair that holds NaN or +inf gives a NaN row.  `scale`: a number or a one-element
    tensor.  Returns a new tensor."""
    dt = torch.float64 if cond.dtype == torch.float64 else torch.float32
    c, u = cond.to(dt), uncond.to(dt)
    lc, lu = c.log_softmax(-1), u.log_softmax(-1)
    g = scale.to(device=c.device, dtype=dt).reshape(()) if isinstance(scale, torch.Tensor) else torch.tensor(float(scale), dtype=dt, device=c.device)
    out = torch.addcmul(lu, g, lc - lu)
    out = out.masked_fill((c == float("-inf")) | (u == float("-inf")), float("-inf"))
    bad = lambda x: (x.isnan() | (x == float("inf"))).any(-1, keepdim=True)
    return out.masked_fill(bad(c) | bad(u), float("nan"))


def guided_step(step, scale):
    """`step` (FlamingoModel._decode_step) as the loops see a model under classifier-free guidance: every call runs the LM on [conditional
    rows ; unconditional rows] - the same tokens, the second half without media (media_locations all zero) - and returns
    guided_logits_torch of the two halves, (rows, V).  The prompt step doubles the rows (the visual features are repeated, never encoded
    twice when generate() has encoded them); the caches it returns are twice the rows wide from then on."""
    def guided(step_ids, ml, am, past, pixel_values, visual_features):
        R = step_ids.shape[0]
        two = lambda t: None if t is None else torch.cat([t, t], dim=0)
        logits, past = step(two(step_ids), torch.cat([ml, torch.zeros_like(ml)], dim=0), two(am), past, two(pixel_values), two(visual_features))
        return guided_logits_torch(logits[:R], logits[R:], scale), past
    return guided


def guided_reorder(reorder_cache):
    """`reorder_cache` (FlamingoModel._reorder_cache) for caches of [conditional ; unconditional] rows: row r + R follows row r."""
    return lambda past, beam_idx: reorder_cache(past, torch.cat([beam_idx, beam_idx + beam_idx.numel()]))


def _dynamic_processor(processors, eos, L0, constraints=None):
    """(logits, sequences so far) -> logits for the dynamic loops: process_logits with the call's settings, then constrain_logits_torch with
    the call's tables; the identity without either."""
    if processors is None and constraints is None:
        return lambda x, s: x
    p = Processors(*processors) if processors is not None else None
    c = constraints

    def process(x, s):
        if p is not None:
            x = process_logits(x, s, p.repetition_penalty, p.no_repeat_ngram_size, eos, p.min_len(L0))
        if c is not None:
            x = constrain_logits_torch(x, s, L0, eos, c.trie, c.bad_words)
        return x
    return process


def _pad_finished(nxt, finished, eos, pad):
    """The eos rule of greedy and sampled decoding: a row that has finished takes `pad`, a row that chose `eos` is finished from now on
    (`finished` is updated in place).  Returns the tokens to append."""
    nxt = torch.where(finished, torch.full_like(nxt, pad), nxt)
    finished.logical_or_(nxt == eos)
    return nxt


# ---- the static path: fixed-shape sessions ----
# Decode sessions hold HIP graphs and raw parameter addresses: they live in a weak side table, not in the model's __dict__, so
# copy.deepcopy(model) / pickling (EMA or evaluation copies) neither see nor try to copy them.  The table is keyed by the model and a
# session refers to its model only WEAKLY (a strong reference from the value would keep the key - and with it the model, its static KV
# cache and the captured graph - alive for ever): `del model` frees all of it.
_DECODE_SESSIONS: "weakref.WeakKeyDictionary" = weakref.WeakKeyDictionary()


def _beam_finalize(state, L0, prompt_ids, nb, pad, *, n_return=None, n_groups=1):
    """The result of a beam search from the state block of ff_beam_step, on the host (numpy only; `state` = BeamState.to_host(), plus
    "length" = the sequences' length after the last step, default: the whole history): per sequence the best finished hypothesis - or, when
    the sequence is not done (the length limit), the best of the hypotheses and the open beams, normalised in float32 by len_norm[length],
    the earlier entry on equal scores - as in the tail of beam_search.  Tokens are read back by following hist_parent
    downwards from the entry's row; rows are padded with `pad` to the longest.  Returns (b, width) int64 on the CPU.
    With `n_return` = n it returns (ids (b * n, width), scores (b * n,) float32): per sequence the n best of the same entries, best first,
    the earlier entry on equal scores, each with the normalised score it was ranked by; where fewer than n entries exist the missing rows
    are all `pad` with score -inf.
    With `n_groups` = G > 1 (the block of ff_group_beam_step) the entries of a sequence are listed group by group, g = 0 .. G - 1: g's
    hypotheses, then g's open beams if g is not done; the ranking is the same stable sort.  Groups may hold the same sequence (the penalty
    is soft), and the scores carry the accumulated penalties."""
    import numpy as np
    G, gs = n_groups, nb // n_groups
    hist_tok, hist_parent, len_norm = state["hist_tok"], state["hist_parent"], state["len_norm"]
    length, eos = int(state.get("length", hist_tok.shape[0])), int(state.get("eos", -1))
    prompt = np.asarray(prompt_ids)

    def backtrack(row, last):               # the tokens at positions L0 .. last of the beam that sat in `row` after the step that wrote `last`
        toks = []
        for p in range(last, L0 - 1, -1):
            toks.append(int(hist_tok[p, row]))
            row = int(hist_parent[p, row])
        return toks[::-1]

    out, scores = [], []
    n_seq = state["score"].shape[0]
    n_hyp, done = np.reshape(state["n_hyp"], (n_seq, G)), np.reshape(state["done"], (n_seq, G))
    for s in range(n_seq):
        hyps = []
        for g in range(G):
            hyps += [(np.float32(state["hyp_score"][s, j]), (int(state["hyp_row"][s, j]), int(state["hyp_len"][s, j]) - 2, [eos]))
                     for j in range(g * gs, g * gs + int(n_hyp[s, g]))]
            if not done[s, g]:
                hyps += [(np.float32(state["score"][s, k]) / np.float32(len_norm[length]), (s * nb + k, length - 1, []))
                         for k in range(g * gs, (g + 1) * gs) if state["score"][s, k] > -np.inf]
        order = sorted(range(len(hyps)), key=lambda j: -hyps[j][0])            # (a stable sort: the earlier entry on equal scores)
        for j in range(1 if n_return is None else n_return):
            if j < len(order):
                row, last, tail = hyps[order[j]][1]
                out.append([int(t) for t in prompt[s]] + backtrack(row, last) + tail)
                scores.append(hyps[order[j]][0])
            else:
                out.append([])
                scores.append(np.float32(-np.inf))
    width = max(len(o) for o in out)
    ids = torch.tensor([o + [pad] * (width - len(o)) for o in out], dtype=torch.long)
    return ids if n_return is None else (ids, torch.from_numpy(np.asarray(scores, np.float32)))


class _DecodeSession:
    """Fixed-shape decoding for one (batch, max_length) shape: the LM keeps a transformers StaticCache of max_length positions, the
    attention mask and the token buffer are preallocated, positions travel as a device tensor (`cache_position`), the cross-attention K / V
    of the prompt step are copied into persistent buffers, and the text_time of a generated token is the prompt's last value (generated
    tokens are never media tags).  A decode step then issues exactly the same work on the same addresses every time, so on the GPU it is
    captured once into a HIP graph and replayed (the eager step is host-bound: 72 layers, ~800 launches of a few microseconds each).
    If the capture raises (e.g. a host synchronisation inside the stock LM) the steps run eagerly.
    This class is what the strategies share - the caches and buffers, the step, capture and replay, the prompt step and the loop of run().
    How a token is chosen is the subclass's: _TokenSession (greedy, sampling) and _BeamSession supply _alloc, _begin, _history, _select,
    _all_done and _result, and override neither _append nor run.  _ContrastiveSession, whose selection needs the LM's output for the
    candidates, also supplies _first and _step.
    `processors` (a Processors) puts functional.process_logits (one launch, csrc/ff_logits.hip) in front of the selection of every strategy:
    _append edits the step's logits in place against the strategy's token history (_history(), with `pos` as its length) and against
    `min_len`, a device scalar _begin sets outside any capture.  A session without processors issues none of this.
    `constraints` (Constraints.caps(): capacities, not contents) puts functional.constrain_logits (one launch, csrc/ff_constrain.hip) behind
    it: the session owns table buffers of those capacities, every call's tables are copied into them before the prompt step together with
    `gen_start` (the prompt's length), outside any capture, and the captured step reads whatever they hold - a later call with other
    candidates of the same capacity class replays the same graph.  A session without constraints allocates and issues none of this.
    `guidance` makes it a classifier-free-guidance session: everything on the LM's side - the StaticCache, `am_buf`, `tt_step`, the
    cross-attention K / V and the LM token buffer `lm_tok` - is 2 R rows wide, [conditional rows ; unconditional rows] (R = b * nb; row r
    pairs with row r + R, the second half is the same ids with media_locations all zero), while everything the strategies own stays R rows.
    _append combines the two halves of a step's logits into `guided` (R, V) float32 with functional.guided_logits (one launch,
    csrc/ff_guidance.hip) and hands THAT to the processors, the constraints and the selection.  The scale is the device scalar `scale`,
    written by run() outside any capture: a later call with another scale replays the same graph.  A session without guidance allocates
    and issues none of this."""

    nb = 1                                 # rows per sequence
    first_in_step = False                  # the prompt step chooses the first token (True: the first decode step does, and one more step runs)
    prompt_kwargs = {}                     # further arguments of the prompt step's forward

    def __init__(self, model, b, max_length, device, ids_dtype, am_dtype, eos, pad, graph, sampling=None, beams=None, processors=None, logprobs=False,
                 constraints=None, groups=None, guidance=False, truncation=None):
        from transformers.cache_utils import StaticCache
        self._model_ref = weakref.ref(model)
        self.sampling, self.beams, self.processors, self.logprobs, self.constraints = sampling, beams, processors, logprobs, constraints
        self.groups, self.guidance, self.truncation = groups, guidance, truncation
        self.n_seq = b
        b = b * self.nb
        lm_b = 2 * b if guidance else b        # rows on the LM's side
        self.b, self.max_length, self.eos, self.graph_wanted = b, max_length, eos, graph
        self.fill = pad if pad is not None else 0
        self.lm_family = model.flamingo.lm_family
        self.cache = StaticCache(config=model.flamingo.lm.config, max_cache_len=max_length)
        self.ids_buf = torch.empty((b, max_length), dtype=ids_dtype, device=device)
        self.am_buf = torch.empty((lm_b, max_length), dtype=am_dtype, device=device)
        self.pos = torch.zeros((1,), dtype=torch.long, device=device)          # position of `tok` (the token the next step consumes)
        self.tok = torch.zeros((b, 1), dtype=ids_dtype, device=device)
        self.tt_step = torch.zeros((lm_b, 1), dtype=torch.int32, device=device)
        if guidance:
            self.lm_tok = torch.zeros((lm_b, 1), dtype=ids_dtype, device=device)
            self.scale = torch.ones((1,), dtype=torch.float32, device=device)
            self.guided = None                                                # (b, V) float32, allocated by the first prompt step
        if constraints is not None:
            self._alloc_constraints()
        self._alloc()
        self.xattn_past = None                                                # persistent (k, v) per layer, filled by every prompt step
        self.replay = None
        self.capture_failed = False
        self.param_ptrs = self._param_ptrs()                                   # what a captured graph reads: checked before every reuse

    @property
    def model(self):
        m = self._model_ref()
        if m is None:
            raise RuntimeError("decode session used after its model was deleted")
        return m

    def _param_ptrs(self):
        return tuple(p.data_ptr() for p in self.model.parameters())

    def stale(self) -> bool:
        """Parameters were re-allocated since this session was built (model.to() / .half(), ShardedAdamW moving them into flat buffers):
        a captured graph would replay reads of freed memory."""
        return self.param_ptrs != self._param_ptrs()

    def _alloc_min_len(self):              # the processors' device scalar; subclasses call it from _alloc when they have processors
        p = self.processors
        self.min_len = torch.zeros((1,), dtype=torch.long, device=self.pos.device)
        self.min_on = self.eos is not None and (p.min_length > 0 or p.min_new_tokens > 0)

    def _alloc_constraints(self):
        _, node_cap, edge_cap, bw_cap, bw_tok_cap = self.constraints
        i32 = lambda n, dt=torch.int32: torch.zeros((n,), dtype=dt, device=self.pos.device)
        self.gen_start = torch.zeros((1,), dtype=torch.long, device=self.pos.device)
        self.trie_bufs = (i32(node_cap + 1), i32(edge_cap), i32(edge_cap), i32(node_cap, torch.uint8), i32(1)) if node_cap else None
        self.bw_bufs = (i32(bw_cap + 1), i32(bw_tok_cap), i32(1)) if bw_cap else None

    def _begin_constraints(self, c, L0):
        """A call's tables into the session's buffers (the live prefix; what lies behind it is never read) and gen_start = the prompt's length."""
        assert c.caps() == self.constraints
        dev = self.pos.device
        put = lambda buf, a: buf[:len(a)].copy_(torch.from_numpy(a).to(dev))
        self.gen_start.fill_(L0)
        if c.trie is not None:
            t = c.trie
            for buf, a in zip(self.trie_bufs, (t.node_first, t.edge_tok, t.edge_child, t.node_terminal)):
                put(buf, a)
            self.trie_bufs[4].fill_(t.n_nodes)
        if c.bad_words is not None:
            w = c.bad_words
            put(self.bw_bufs[0], w.bw_off)
            put(self.bw_bufs[1], w.bw_tok)
            self.bw_bufs[2].fill_(w.n)

    def _append(self, logits):
        """The single place that receives a step's unprocessed logits: under guidance the two halves become the guided scores, then the
        processors, then the constraints, in place, against the first `pos` tokens of every row of the strategy's history, then the
        strategy's selection."""
        p = self.processors
        if self.guidance:
            if self.guided is None:                                           # (the prompt step: never inside a capture)
                self.guided = torch.empty((self.b, logits.shape[-1]), dtype=torch.float32, device=logits.device)
            logits = F.guided_logits(logits[:self.b], logits[self.b:], self.scale, out=self.guided)
        if p is not None:
            F.process_logits(logits, self._history(), self.pos, p.repetition_penalty, p.no_repeat_ngram_size, self.eos if self.min_on else None, self.min_len if self.min_on else None)
        if self.constraints is not None:
            F.constrain_logits(logits, self._history(), self.pos, self.gen_start, self.eos, trie=self.trie_bufs, bad_words=self.bw_bufs)
        self._select(logits)

    def _first(self, out):                 # what the prompt step's output feeds
        self._append(out.logits[:, -1])

    def _positions(self, L0=None):
        """How the LM family learns where a step's tokens sit without reading anything back to the host.  GPT-2 takes absolute cache
        positions.  OPT numbers the ATTENDED tokens (cumsum of the attention mask, padding skipped - modeling_opt's own rule), and derives
        that by slicing with the cache's length, which for a StaticCache is a device scalar (a host synchronisation: not capturable): the
        decode step hands it `position_ids` instead - the token at `pos` is the (number of ones in the mask so far)-th attended one."""
        if self.lm_family == "gpt2":
            return {"cache_position": self.pos if L0 is None else torch.arange(L0, device=self.pos.device)}
        if L0 is None:
            return {"position_ids": self.am_buf.sum(1, keepdim=True).long() - 1}
        return {}                       # the prompt step: an empty cache, OPT's own cumsum applies

    def _step(self):
        self.am_buf.index_fill_(1, self.pos, 1)
        if self.guidance:
            self.lm_tok.view(2, self.b, 1).copy_(self.tok)                   # both halves consume the chosen token
        o = self.model.flamingo(input_ids=self.lm_tok if self.guidance else self.tok, attention_mask=self.am_buf, use_cache=True, past_key_values=(self.xattn_past, self.cache),
                                text_time=self.tt_step, **self._positions())
        self.pos.add_(1)
        self._append(o.logits[:, -1])

    @torch.no_grad()
    def run(self, ids, ml, am, pixel_values, visual_features, generator=None, n_return=None, constraints=None, guidance_scale=None):
        L0, prompt_ids = ids.shape[1], ids
        ids, ml, am, pixel_values, visual_features = self._begin(ids, ml, am, pixel_values, visual_features, generator)
        if self.constraints is not None:
            self._begin_constraints(constraints, L0)
        lm_ids = ids
        if self.guidance:                                                     # [conditional ; unconditional]: the same ids, the second half without media
            self.scale.fill_(guidance_scale)
            if visual_features is None and pixel_values is not None:         # encoded once, repeated
                visual_features, pixel_values = self.model.flamingo.encode_resample_visuals(pixel_values), None
            lm_ids, ml, am = torch.cat([ids, ids]), torch.cat([ml, torch.zeros_like(ml)]), torch.cat([am, am])
            if visual_features is not None:
                visual_features = torch.cat([visual_features, visual_features])
        self.cache.reset()
        out = self.model.flamingo(input_ids=lm_ids, attention_mask=am, media_locations=ml, use_cache=True, past_key_values=(None, self.cache),
                                  pixel_values=pixel_values, visual_features=visual_features, **self._positions(L0), **self.prompt_kwargs)
        fresh = out.past_key_values[0]
        if self.xattn_past is None:
            self.xattn_past = tuple((torch.empty_like(k, memory_format=torch.contiguous_format), torch.empty_like(v, memory_format=torch.contiguous_format))
                                    for k, v in fresh)
        for (kb, vb), (k, v) in zip(self.xattn_past, fresh):
            kb.copy_(k); vb.copy_(v)
        self.tt_step.copy_(F.text_time(ml)[:, -1:])
        self.ids_buf.fill_(self.fill)
        self.ids_buf[:, :L0] = ids
        self.am_buf.zero_()
        self.am_buf[:, :L0] = am
        self.pos.fill_(L0)
        self._first(out)
        remaining = self.max_length - L0 - 1 + int(self.first_in_step)
        if self.graph_wanted and self.replay is None and not self.capture_failed and remaining > 1:
            self._step()                                                      # eager once: lazy initialisation, allocator pools
            remaining -= 1
            try:
                # captured on a stream whose sync buffer exists before the capture: an unprepared capture would keep the separate to_out
                # launches where the eager steps exchange inside the fused launch (> 32 rows) - replay and eager steps must be the same work
                self.capture_stream = _prepared_capture_stream(self.model)
                g = torch.cuda.CUDAGraph()
                torch.cuda.synchronize()
                with torch.cuda.graph(g, stream=self.capture_stream):
                    self._step()
                self.graph, self.replay = g, g.replay
            except Exception:                                                 # the steps run eagerly from here on (and in later calls)
                torch.cuda.synchronize()
                self.capture_failed = True
        run_step = self.replay or self._step
        i = 0
        all_done = self._all_done()
        while i < remaining:
            run_step()
            i += 1
            if self.eos is not None and i % 16 == 0 and bool(all_done.all()):          # (a host sync: only every 16 tokens)
                break
        return self._result(L0, prompt_ids, self.max_length - remaining + i, n_return)


class _TokenSession(_DecodeSession):
    """Greedy and sampled decoding: one token per row and step, the eos bookkeeping of dynamic_decode.  Token-for-token equal to the
    growing-cache loop when greedy (tests/test_model_plumbing.py).
    `sampling` (a Sampling) makes it a SAMPLING session (GPU only): _select draws the token with functional.sample_tokens (one launch on
    the logits in their own dtype, csrc/ff_sample.hip) instead of the argmax.  The random numbers of a whole call are drawn before the
    prompt step, outside any capture, into `u_all` (max_length, b): row `pos` serves the token written at position `pos` and the captured
    step picks it with a device-side index_select on `pos`, so the graph holds no random-number generation and eager and replayed steps
    consume identical numbers.  The processors read `ids_buf`, which already is the sequence.
    `truncation` (a Truncation, with `sampling`) hands min_p / typical_p / epsilon_cutoff / eta_cutoff to the same call, which then is the
    one launch of csrc/ff_truncate.hip; the values are launch constants of the captured step.  A session without it calls sample_tokens as
    it always did.
    `logprobs` makes _select record the chosen token's log-probability (functional.token_logprobs on the processed logits, one launch inside
    the captured step) into column `pos` of `lp_buf` (b, max_length) float32; a session without it allocates neither buffer and never
    calls the function."""

    def _alloc(self):
        dev = self.pos.device
        self.finished = torch.zeros(self.b, dtype=torch.bool, device=dev)
        self.n_new = torch.zeros((), dtype=torch.long, device=dev)            # tokens appended while not every sequence had finished
        if self.sampling is not None:
            self.u_all = torch.zeros((self.max_length, self.b), dtype=torch.float32, device=dev)
            self.nxt = torch.zeros((self.b,), dtype=torch.long, device=dev)
        if self.processors is not None:
            self._alloc_min_len()
        if self.logprobs:
            self.lp_step = torch.zeros((self.b,), dtype=torch.float32, device=dev)
            self.lp_buf = torch.zeros((self.b, self.max_length), dtype=torch.float32, device=dev)

    def _begin(self, ids, ml, am, pixel_values, visual_features, generator):
        if self.sampling is not None:
            self.u_all.copy_(torch.rand((self.max_length, self.b), generator=generator, device=ids.device, dtype=torch.float32))
        self.finished.zero_()
        self.n_new.zero_()
        if self.processors is not None:
            self.min_len.fill_(self.processors.min_len(ids.shape[1]))
        if self.logprobs:
            self.lp_buf.zero_()
        return ids, ml, am, pixel_values, visual_features

    def _history(self):
        return self.ids_buf

    def _select(self, logits):             # choose, apply the eos bookkeeping, append at `pos`
        if self.sampling is None:
            nxt = logits.float().argmax(-1)
        elif self.truncation is None:
            nxt = F.sample_tokens(logits, self.u_all.index_select(0, self.pos).view(-1), *self.sampling, out=self.nxt)
        else:
            nxt = F.sample_tokens(logits, self.u_all.index_select(0, self.pos).view(-1), *self.sampling, out=self.nxt, **self.truncation._asdict())
        if self.logprobs:                  # the chosen token's log-softmax, 0 for a row that had finished (one launch, csrc/ff_logprob.hip);
            # `finished` still is what it was before this step: _pad_finished below updates it after the launch, in stream order
            F.token_logprobs(logits, nxt, skip=self.finished, out=self.lp_step)
            self.lp_buf.index_copy_(1, self.pos, self.lp_step[:, None])
        alive = ~self.finished.all()
        if self.eos is not None:
            nxt = _pad_finished(nxt, self.finished, self.eos, self.fill)
        self.tok.copy_(nxt[:, None])
        self.ids_buf.index_copy_(1, self.pos, self.tok)
        self.n_new.add_(alive.to(self.n_new.dtype))

    def _all_done(self):
        return self.finished

    def _result(self, L0, prompt_ids, length, n_return=None):
        ids = self.ids_buf[:, :L0 + int(self.n_new)].clone() if self.eos is not None else self.ids_buf.clone()
        return (ids, self.lp_buf[:, L0:ids.shape[1]].clone()) if self.logprobs else ids


class _BeamSession(_DecodeSession):
    """Beam search (GPU only) for `b` sequences with `beams` (a Beams): every buffer and the LM cache are b * nb rows wide (row s * nb + k =
    beam k of sequence s; the visual features are encoded once per sequence and repeated), and _select is functional.beam_step (selection
    and all bookkeeping in a device state block, csrc/ff_beam.hip), functional.beam_gather (the static LM cache reordered in place by beam
    index, live positions only) and tok <- next_tok.  The cross-attention K / V, the attention mask and text_time are equal within a
    sequence's beams and are NOT reordered.  The result is read back once, after the loop (_beam_finalize).
    The processors read `seq_buf` (b * nb, max_length), which follows the beams through the same in-place gather as the LM cache (viewed as
    two 4-byte elements per id), and so do the constraints: a beam's position in the trie is a function of its own tokens.  A session with
    neither allocates no seq_buf.
    `groups` (a Groups) makes it DIVERSE beam search: the state block is built with n_groups, _select calls functional.group_beam_step with
    the penalty as a launch constant, and everything else - the gathers, seq_buf, the processors, the constraints - acts per row and is what
    it was.  A session without groups calls beam_step.
    Under `guidance` the LM cache is 2 b * nb rows and is gathered with a preallocated doubled index (beam_idx, then beam_idx + b * nb,
    filled inside the step): ff_beam_gather maps within each run of nb rows, so the unconditional half follows its beams; seq_buf and the
    state block stay b * nb rows.
    `sampling` (a Sampling, beside `beams`) makes it BEAM SAMPLING: _select calls functional.beam_sample_step - the selection draws 2 nb
    continuations per sequence by a Gumbel top-k whose noise is a function of (seed, cur_len, row, column), recomputed inside the kernel -
    with temperature / top_k / top_p as launch constants and `seed`, a device int64 that _begin fills from the call's generator with one
    torch.randint outside the capture.  Eager and replayed steps therefore draw the same numbers; everything else - the gathers, seq_buf,
    the processors, the constraints, guidance - is what it was.  A session without sampling holds no seed and calls beam_step."""

    def __init__(self, model, b, *args, beams, **kw):
        self.nb = beams.nb
        super().__init__(model, b, *args, beams=beams, **kw)

    def _alloc(self):
        dev = self.pos.device
        self.state = F.BeamState(self.n_seq, self.nb, self.max_length, dev, eos=self.eos, pad=self.fill, early_stopping=self.beams.early_stopping, length_penalty=self.beams.length_penalty,
                                 **({"n_groups": self.groups.n} if self.groups is not None else {}))
        self.cur_len = torch.zeros((1,), dtype=torch.long, device=dev)        # pos + 1: the length after the token beam_step chooses
        self.lm_tensors = None                                                # keys / values of every StaticCache layer (allocated by the first prompt step)
        if self.processors is not None:
            self._alloc_min_len()
        if self.sampling is not None:
            self.seed = torch.zeros((1,), dtype=torch.long, device=dev)      # what the step's noise is a function of, beside cur_len, row and column
        if self.guidance:
            self.lm_beam_idx = torch.zeros((2 * self.b,), dtype=torch.long, device=dev)      # beam_idx, then beam_idx + R: the unconditional half follows
        if self.processors is not None or self.constraints is not None:
            self.seq_buf = torch.full((self.b, self.max_length), self.fill, dtype=torch.long, device=dev)

    def _begin(self, ids, ml, am, pixel_values, visual_features, generator):
        if visual_features is None and pixel_values is not None:             # encoded once per sequence, repeated per beam
            visual_features, pixel_values = self.model.flamingo.encode_resample_visuals(pixel_values), None
        ids, ml, am = _repeat_leading(ids, self.nb), _repeat_leading(ml, self.nb), _repeat_leading(am, self.nb)
        if visual_features is not None:
            visual_features = _repeat_leading(visual_features, self.nb)
        self.state.reset()
        if self.sampling is not None:                                         # one draw per call, outside any capture: the replayed step only reads it
            self.seed.copy_(torch.randint(0, 2 ** 63 - 1, (1,), generator=generator, device=ids.device, dtype=torch.long))
        if self.processors is not None:
            self.min_len.fill_(self.processors.min_len(ids.shape[1]))
        if hasattr(self, "seq_buf"):
            self.seq_buf.fill_(self.fill)
            self.seq_buf[:, :ids.shape[1]] = ids
        return ids, ml, am, pixel_values, visual_features

    def _history(self):
        return self.seq_buf

    def _select(self, logits):
        if self.lm_tensors is None:
            self.lm_tensors = [t for layer in self.cache.layers for t in (layer.keys, layer.values)]
        torch.add(self.pos, 1, out=self.cur_len)
        if self.sampling is not None:
            nxt, beam_idx = F.beam_sample_step(logits, self.state, self.cur_len, self.seed, *self.sampling)
        elif self.groups is None:
            nxt, beam_idx = F.beam_step(logits, self.state, self.cur_len)
        else:
            nxt, beam_idx = F.group_beam_step(logits, self.state, self.cur_len, self.groups.diversity_penalty)
        if self.guidance:
            self.lm_beam_idx[:self.b].copy_(beam_idx)
            torch.add(beam_idx, self.b, out=self.lm_beam_idx[self.b:])
        F.beam_gather(self.lm_tensors, self.lm_beam_idx if self.guidance else beam_idx, self.pos, self.nb)           # positions < pos are live: the cache rows follow their beams
        if hasattr(self, "seq_buf"):                                          # ... and so do the histories: an id is two 4-byte elements
            F.beam_gather([self.seq_buf.view(torch.int32).view(self.b, 1, self.max_length, 2)], beam_idx, self.pos, self.nb)
            self.seq_buf.index_copy_(1, self.pos, nxt[:, None])
        self.tok.copy_(nxt[:, None])

    def _all_done(self):
        return self.state.done

    def _result(self, L0, prompt_ids, length, n_return=None):    # one device-to-host copy; steps past the last `done` only wrote padding
        host = self.state.to_host()
        host["length"] = length
        res = _beam_finalize(host, L0, prompt_ids.cpu(), self.nb, self.fill, n_return=n_return, **({"n_groups": self.groups.n} if self.groups is not None else {}))
        return res.to(prompt_ids.device) if n_return is None else tuple(t.to(prompt_ids.device) for t in res)


class _ContrastiveSession(_DecodeSession):
    """Contrastive search (GPU only) for `b` sequences with `contrastive` (a Contrastive): rules T and C1 - C9 of include/flamingo_fusion.h.
    Every LM-side buffer and the LM cache are b * k rows wide (row s * k + c = candidate c of sequence s; the prompt is repeated k times, the
    visual features are encoded once per sequence and repeated, as in _BeamSession); `tok` holds the CANDIDATES, so a decode step runs the LM
    on all of them (rule C1).  The session owns `hist` (b, max_length, dim), the lm_head inputs of the positions so far, in the model's dtype;
    `mask` (b, max_length) - the prompt's attention mask, 1 from the prompt's end on, written by _begin outside any capture -; `seq_buf`
    (b, max_length), the sequences, which is what the processors and constraints read; `next_logits` (b, V), the chosen rows' logits, which
    they edit in place; the candidate buffers `cand_tok` / `cand_logp` (b, k); `alpha`, a device scalar run() writes outside any capture - a
    later call with another penalty_alpha replays the same graph -; `finished`, `n_new` and, with `logprobs`, `lp_buf`.
    The prompt step fills hist[:, :L0] from the rows s * k, runs the processors, the constraints and functional.topk_logprobs on those rows'
    logits and writes tok <- candidates: it chooses NO token.  A decode step is: the LM on the b * k candidates; functional.contrastive_step
    (one launch: the look-ahead ranking, the choice, the eos bookkeeping, hist[:, pos] <- the chosen vector); functional.beam_gather of the LM
    cache with beam_idx - every row of a sequence takes the chosen row, live positions including the one just written -; the token appended to
    seq_buf; index_select(logits, sel_row, out=next_logits); the processors and constraints in place against seq_buf; topk_logprobs;
    tok <- candidates.  The first token is chosen by the first decode step, so a call that fills max_length runs max_length - L0 decode
    steps, one more than the other sessions (first_in_step)."""

    first_in_step = True
    prompt_kwargs = {"output_last_hidden_state": True}

    def __init__(self, model, b, *args, contrastive, **kw):
        self.nb = contrastive.k
        self.contrastive = contrastive
        super().__init__(model, b, *args, **kw)

    def _alloc(self):
        dev, n, k = self.pos.device, self.n_seq, self.nb
        self.finished = torch.zeros(n, dtype=torch.bool, device=dev)
        self.n_new = torch.zeros((), dtype=torch.long, device=dev)            # tokens appended while not every sequence had finished
        self.alpha = torch.zeros((1,), dtype=torch.float32, device=dev)
        self.mask = torch.zeros((n, self.max_length), dtype=torch.bool, device=dev)
        self.seq_buf = torch.full((n, self.max_length), self.fill, dtype=torch.long, device=dev)
        self.cand_tok = torch.zeros((n, k), dtype=torch.long, device=dev)
        self.cand_logp = torch.zeros((n, k), dtype=torch.float32, device=dev)
        self.step_out = (torch.zeros((n,), dtype=torch.long, device=dev), torch.zeros((n,), dtype=torch.float32, device=dev),
                         torch.zeros((n,), dtype=torch.long, device=dev), torch.zeros((n * k,), dtype=torch.long, device=dev))      # next_tok, logprob, sel_row, beam_idx
        self.hist = self.next_logits = self.lm_tensors = None                 # allocated by the first prompt step (the model says dim, V and the dtypes)
        if self.processors is not None:
            self._alloc_min_len()
        if self.logprobs:
            self.lp_buf = torch.zeros((n, self.max_length), dtype=torch.float32, device=dev)

    def _begin(self, ids, ml, am, pixel_values, visual_features, generator):
        L0 = ids.shape[1]
        if visual_features is None and pixel_values is not None:             # encoded once per sequence, repeated per candidate
            visual_features, pixel_values = self.model.flamingo.encode_resample_visuals(pixel_values), None
        self.finished.zero_()
        self.n_new.zero_()
        self.mask.fill_(True)
        self.mask[:, :L0] = am != 0
        self.seq_buf.fill_(self.fill)
        self.seq_buf[:, :L0] = ids
        if self.processors is not None:
            self.min_len.fill_(self.processors.min_len(L0))
        if self.logprobs:
            self.lp_buf.zero_()
        ids, ml, am = _repeat_leading(ids, self.nb), _repeat_leading(ml, self.nb), _repeat_leading(am, self.nb)
        if visual_features is not None:
            visual_features = _repeat_leading(visual_features, self.nb)
        return ids, ml, am, pixel_values, visual_features

    def _history(self):
        return self.seq_buf

    def _first(self, out):                 # the prompt step: H[:, :L0] and the first candidates, from the rows s * k
        h, logits = out.hidden_states[-1][::self.nb], out.logits[::self.nb, -1]
        if self.hist is None:
            self.hist = torch.zeros((self.n_seq, self.max_length, h.shape[-1]), dtype=h.dtype, device=h.device)
            self.next_logits = torch.empty((self.n_seq, logits.shape[-1]), dtype=logits.dtype, device=logits.device)
            self.lm_tensors = [t for layer in self.cache.layers for t in (layer.keys, layer.values)]
        self.hist[:, :h.shape[1]].copy_(h)
        self.next_logits.copy_(logits)
        self._append(self.next_logits)

    def _select(self, logits):             # rule T on the processed logits of the chosen rows; the candidates are what the next step feeds
        F.topk_logprobs(logits, self.nb, out=(self.cand_tok, self.cand_logp))
        self.tok.copy_(self.cand_tok.view(-1, 1))

    def _step(self):
        self.am_buf.index_fill_(1, self.pos, 1)
        o = self.model.flamingo(input_ids=self.tok, attention_mask=self.am_buf, use_cache=True, past_key_values=(self.xattn_past, self.cache),
                                text_time=self.tt_step, output_last_hidden_state=True, **self._positions())
        nxt, lp, sel_row, beam_idx = self.step_out
        alive = ~self.finished.all()                                          # (before the launch updates `finished`, in stream order)
        F.contrastive_step(o.hidden_states[-1][:, -1], self.hist, self.mask, self.cand_tok, self.cand_logp, self.finished, self.alpha, self.pos,
                           eos=self.eos, pad=self.fill, out=self.step_out)
        self.seq_buf.index_copy_(1, self.pos, nxt[:, None])
        if self.logprobs:
            self.lp_buf.index_copy_(1, self.pos, lp[:, None])
        self.n_new.add_(alive.to(self.n_new.dtype))
        self.pos.add_(1)
        F.beam_gather(self.lm_tensors, beam_idx, self.pos, self.nb)          # positions < pos are live, the one just written included
        torch.index_select(o.logits[:, -1], 0, sel_row, out=self.next_logits)
        self._append(self.next_logits)

    @torch.no_grad()
    def run(self, *args, penalty_alpha, **kw):
        self.alpha.fill_(penalty_alpha)                                       # outside any capture: the replayed step only reads it
        return super().run(*args, **kw)

    def _all_done(self):
        return self.finished

    def _result(self, L0, prompt_ids, length, n_return=None):
        ids = self.seq_buf[:, :L0 + int(self.n_new)].clone() if self.eos is not None else self.seq_buf.clone()
        ids = ids.to(prompt_ids.dtype)
        return (ids, self.lp_buf[:, L0:ids.shape[1]].clone()) if self.logprobs else ids


def _static_decode(model, ids, ml, am, pixel_values, visual_features, max_length, eos, pad, sampling=None, generator=None, beams=None, processors=None,
                   logprobs=False, n_return=None, constraints=None, groups=None, guidance=None, truncation=None, contrastive=None):
    """Greedy, sampled (`sampling`) or beam-search (`beams`) decoding with FIXED shapes (see _DecodeSession).  Sessions - preallocated caches
    and buffers plus, on the GPU, the captured HIP graph of one decode step - are kept per (batch, max_length, keys per sequence, device,
    eos, pad, graph, sampling, beams, processors) and reused by later calls, so only the first caption batch of a shape pays for the
    capture.  A session whose model's parameters were re-allocated since (model.to(), ShardedAdamW) is rebuilt;
    FlamingoModel.reset_decode_sessions() drops them all.
    `logprobs` (greedy and sampling) selects a session that records the chosen tokens' log-probabilities: its key is the same ten elements
    followed by "logprobs", and the call returns (ids, token_logprobs).  `n_return` (beam search) returns (ids, scores) with the n best
    entries per sequence (_beam_finalize); it changes nothing in the session.  `constraints` (a Constraints) selects a session that decodes
    under a candidate trie and / or banned words: its key ends with Constraints.caps() - the tables' capacities, not their contents.
    `groups` (a Groups, with `beams`) selects a diverse-beam-search session: its key ends with the Groups - the penalty is a launch constant of
    the captured step.  A call without groups builds the key it always built.
    `guidance` (the scale, a float) selects a classifier-free-guidance session: its key ends with "guidance", NOT with the scale, which is
    a device scalar the captured step reads - a sweep over scales replays one graph.  A call without it builds the key it always built.
    `truncation` (a Truncation, with `sampling`) selects a session that samples under min_p / typical_p / epsilon_cutoff / eta_cutoff: its
    key ends with the Truncation - the values are launch constants of the captured step, like the Groups.  A call without it builds the key it
    always built.
    `sampling` TOGETHER with `beams` selects a beam-sampling session (a _BeamSession whose selection draws): the key's own `sampling` and
    `beams` elements tell it from both, nothing is appended.
    `contrastive` (a Contrastive) selects a _ContrastiveSession: its key ends with ("contrastive", k) - the k, which is the session's shape,
    NOT penalty_alpha, a device scalar the captured step reads: a sweep over alpha replays one graph.  A call without it builds the key it
    always built."""
    b = ids.shape[0]
    graph = ids.is_cuda and not model.training and model.decode_graph
    sessions = _DECODE_SESSIONS.setdefault(model, {})
    n_media = int(ml.sum(-1).max()) if visual_features is None and pixel_values is None else \
        (visual_features.shape[1] if visual_features is not None else (pixel_values.shape[1] if pixel_values.ndim >= 5 else pixel_values.shape[0]))
    key = (b, max_length, n_media, str(ids.device), eos, pad, bool(graph), sampling, beams, processors) + (("logprobs",) if logprobs else ())
    if constraints is not None:
        key += (constraints.caps(),)
    if groups is not None:
        key += (groups,)
    if guidance is not None:
        key += ("guidance",)
    if truncation is not None:
        key += (truncation,)
    if contrastive is not None:
        key += (("contrastive", contrastive.k),)
    sess = sessions.get(key)
    if sess is not None and sess.stale():
        sessions.pop(key)
        sess = None
    if sess is None:
        if len(sessions) >= 4:                                                # a handful of shapes at most: each holds a KV cache and a graph
            sessions.pop(next(iter(sessions)))
        cls = _ContrastiveSession if contrastive is not None else (_TokenSession if beams is None else _BeamSession)
        sess = sessions[key] = cls(model, b, max_length, ids.device, ids.dtype, am.dtype, eos, pad, graph, sampling=sampling, beams=beams, processors=processors, logprobs=logprobs,
                                   **({"constraints": constraints.caps()} if constraints is not None else {}), **({"groups": groups} if groups is not None else {}),
                                   **({"guidance": True} if guidance is not None else {}), **({"truncation": truncation} if truncation is not None else {}),
                                   **({"contrastive": contrastive} if contrastive is not None else {}))
    return sess.run(ids, ml, am, pixel_values, visual_features, generator=generator, n_return=n_return, **({"constraints": constraints} if constraints is not None else {}),
                    **({"guidance_scale": guidance} if guidance is not None else {}), **({"penalty_alpha": contrastive.penalty_alpha} if contrastive is not None else {}))


# ---- the dynamic path: growing caches, one forward per step (the only path on CPU tensors, and what the sessions are tested against) ----
def dynamic_decode(step, ids, ml, am, pixel_values, visual_features, max_length, eos, pad, sampling=None, generator=None, processors=None,
                   logprob_dtype=None, constraints=None, truncation=None):
    """Greedy or, with `sampling`, multinomial decoding over the cached decode path; `step` is FlamingoModel._decode_step.
    With `truncation` (a Truncation) the filtered logits also pass truncate_logits_torch before the draw; without it nothing changes.
    With `logprob_dtype` (torch.float32, or torch.float64 for a model that computes in float64) it returns (ids, token_logprobs): the
    log-softmax of the processed logits at the chosen token, taken in that dtype, 0 for a row that had finished before the step."""
    finished = torch.zeros(ids.shape[0], dtype=torch.bool, device=ids.device)
    lps = []
    past, step_ids = None, ids
    process = _dynamic_processor(processors, eos, ids.shape[1], constraints)
    while ids.shape[1] < max_length:
        logits, past = step(step_ids, ml, am, past, pixel_values, visual_features)
        logits = process(logits, ids)
        if sampling is not None and truncation is not None:
            nxt = torch.multinomial(truncate_logits_torch(filter_logits(logits, *sampling), *truncation).softmax(-1), 1, generator=generator)[:, 0]
        elif sampling is not None:
            nxt = torch.multinomial(filter_logits(logits, *sampling).softmax(-1), 1, generator=generator)[:, 0]
        else:
            nxt = logits.argmax(-1)
        if logprob_dtype is not None:
            lp = logits.to(logprob_dtype).log_softmax(-1).gather(1, nxt[:, None])[:, 0]
            lps.append(torch.where(finished, torch.zeros_like(lp), lp))
        if eos is not None:
            nxt = _pad_finished(nxt, finished, eos, pad)
        ids = torch.cat([ids, nxt[:, None]], dim=1)
        ml = torch.cat([ml, torch.zeros_like(ml[:, :1])], dim=1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], dim=1)
        step_ids = ids[:, -1:]
        if eos is not None and bool(finished.all()):
            break
    if logprob_dtype is not None:
        return ids, (torch.stack(lps, dim=1) if lps else torch.zeros((ids.shape[0], 0), dtype=logprob_dtype, device=ids.device))
    return ids


def beam_search(step, reorder_cache, ids, ml, am, pixel_values, visual_features, max_length, nb, eos, pad, early_stopping, length_penalty, processors=None,
                n_return=None, constraints=None, groups=None, sampling=None, generator=None, noise=None):
    """Standard beam search over the cached decode path; `step` / `reorder_cache` are FlamingoModel._decode_step / ._reorder_cache.  The
    prompt runs once per sequence; its caches are then replicated per beam (xattn K/V: repeat_interleave; LM cache:
    Cache.batch_repeat_interleave) and re-ordered every step.  `processors` act on every step's logits before the log-softmax.
    With `n_return` = n it returns (ids (b * n, width), scores (b * n,) float32): per sequence the n best of what the tail ranks, best first,
    the earlier entry on equal scores, with their normalised scores; missing rows are all pad with score -inf (as _beam_finalize).
    With `groups` (a Groups) it is DIVERSE beam search, rules A - D of ff_group_beam_step (include/flamingo_fusion.h) restated in torch: the
    nb beams are G groups of gs, inside a step the groups are searched in order, and a group's candidates pay the penalty for every live next
    beam of an earlier group that carries their token (the product and the difference rounded in float32); each group has its own
    hypotheses and done flag, and the tail ranks all groups' entries together.  It also runs on CPU tensors.  Without groups nothing
    changes: one group of nb beams, the same topk, the same calls.
    With `sampling` (a Sampling; not with groups) it is BEAM SAMPLING, rules S1 - S6 of ff_beam_sample_step restated in torch
    (beam_sample_select_torch, order_by_score): every step draws its 2 nb candidates without replacement by a Gumbel top-k on the warped,
    accumulated scores, with noise from gumbel_noise_torch(generator=) - a different stream than the static path's Philox, as with token
    sampling - or, for tests, from `noise(rows, V, cur_len)`.  It also runs on CPU tensors.  Without sampling nothing changes."""
    b, L0 = ids.shape
    dev = ids.device
    process = _dynamic_processor(processors, eos, L0, constraints)
    logits, past = step(ids, ml, am, None, pixel_values, visual_features)
    x = process(logits, ids)
    logp = x.log_softmax(-1)
    V = logp.shape[-1]
    xattn_past, lm_past = past
    xattn_past = tuple(tuple(_repeat_leading(t, nb) for t in kv) for kv in xattn_past)
    if hasattr(lm_past, "batch_repeat_interleave"):
        lm_past.batch_repeat_interleave(nb)
    else:
        lm_past = tuple(tuple(_repeat_leading(t, nb) for t in layer) for layer in lm_past)
    past = (xattn_past, lm_past)
    seqs = _repeat_leading(ids, nb)                                   # (b * nb, L)
    ml, am = _repeat_leading(ml, nb), _repeat_leading(am, nb)
    G, lam = (groups.n, torch.tensor(groups.diversity_penalty, dtype=torch.float32)) if groups is not None else (1, None)
    gs = nb // G                                                      # beams per group (no groups: one group of nb)
    scores = torch.full((b, nb), float("-inf"), device=dev)
    scores[:, ::gs] = 0.0                                             # all beams of a group start identical: only one may branch
    logp = _repeat_leading(logp, nb)
    x = _repeat_leading(x, nb) if sampling is not None else None      # the processed logits: what rule S1 starts from
    done_hyps = [[[] for _ in range(G)] for _ in range(b)]            # (normalised score, token list) per sequence and group
    is_done = [[False] * G for _ in range(b)]
    while True:
        cand = (scores.reshape(-1, 1) + logp).reshape(b, nb * V)
        cur_len = seqs.shape[1] + 1
        next_scores = torch.full((b, nb), float("-inf"), device=dev)
        next_tok = torch.full((b, nb), pad if pad is not None else 0, dtype=torch.long, device=dev)
        next_src = torch.arange(nb, device=dev).repeat(b, 1)
        if sampling is not None:
            g = noise(b * nb, V, cur_len) if noise is not None else gumbel_noise_torch((b * nb, V), generator, dev)
            top_s, top_i = order_by_score(*beam_sample_select_torch(x, scores, g, nb, *sampling), V)
            top_s_c, top_i_c = top_s.to(torch.float32).cpu(), top_i.cpu()
        elif groups is None:
            top_s, top_i = cand.topk(2 * nb, dim=-1)
            top_s_c, top_i_c = top_s.cpu(), top_i.cpu()
        else:
            cand_c = cand.cpu().reshape(b, nb, V)
        for bi in range(b):
            chosen = {}                                               # token -> live next beams of the earlier groups that carry it (rule A's c)
            for g in range(G):
                if is_done[bi][g]:
                    continue
                if groups is not None:                                # rule A, then rule B's order: score, then row, then column (a stable sort)
                    x = cand_c[bi, g * gs:(g + 1) * gs].clone()
                    for tok, c in chosen.items():
                        x[:, tok] = x[:, tok] - lam * float(c)
                    top_s_g, top_i_g = x.reshape(-1).sort(descending=True, stable=True)
                    ranked = zip(top_s_g[:2 * gs].tolist(), top_i_g[:2 * gs].tolist())
                else:
                    ranked = zip(top_s_c[bi].tolist(), top_i_c[bi].tolist())
                hyps_g, k = done_hyps[bi][g], g * gs
                for rank, (s_, i_) in enumerate(ranked):
                    beam, tok = g * gs + i_ // V, i_ % V
                    if eos is not None and tok == eos:
                        if rank < gs:
                            hyps_g.append((s_ / (cur_len ** length_penalty), seqs[bi * nb + beam].tolist() + [tok]))
                        continue
                    next_scores[bi, k], next_tok[bi, k], next_src[bi, k] = s_, tok, beam
                    k += 1
                    if k == (g + 1) * gs:
                        break
                if len(hyps_g) >= gs:
                    hyps_g[:] = sorted(hyps_g, key=lambda t: -t[0])[:gs]
                    best_open = float(next_scores[bi, g * gs:(g + 1) * gs].max()) / (cur_len ** length_penalty)
                    if early_stopping or hyps_g[-1][0] >= best_open:
                        is_done[bi][g] = True
                for k in range(g * gs, (g + 1) * gs if groups is not None else 0):
                    if float(next_scores[bi, k]) > float("-inf"):
                        chosen[int(next_tok[bi, k])] = chosen.get(int(next_tok[bi, k]), 0) + 1
        beam_idx = (next_src + torch.arange(b, device=dev)[:, None] * nb).reshape(-1)
        seqs = torch.cat([seqs.index_select(0, beam_idx), next_tok.reshape(-1, 1)], dim=1)
        scores = next_scores
        if all(all(d) for d in is_done) or seqs.shape[1] >= max_length:
            break
        past = reorder_cache(past, beam_idx)
        ml = torch.cat([ml, torch.zeros_like(ml[:, :1])], dim=1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], dim=1)
        logits, past = step(seqs[:, -1:], ml, am, past, None, None)
        x = process(logits, seqs)
        logp = x.log_softmax(-1)
    out, out_scores = [], []
    for bi in range(b):
        hyps = []
        for g in range(G):                                            # rule D: group by group, a group's hypotheses, then its open beams
            hyps += done_hyps[bi][g]
            if not is_done[bi][g]:                                    # length limit: the open beams count as hypotheses too
                hyps += [(float(scores[bi, k]) / (seqs.shape[1] ** length_penalty), seqs[bi * nb + k].tolist()) for k in range(g * gs, (g + 1) * gs)
                         if float(scores[bi, k]) > float("-inf")]
        if n_return is None:
            out.append(max(hyps, key=lambda t: t[0])[1])
            continue
        ranked = sorted(hyps, key=lambda t: -t[0])[:n_return]         # (a stable sort: the earlier entry on equal scores)
        ranked += [(float("-inf"), [])] * (n_return - len(ranked))
        out += [h[1] for h in ranked]
        out_scores += [h[0] for h in ranked]
    width = max(len(o) for o in out)
    fill = pad if pad is not None else 0
    ids = torch.tensor([o + [fill] * (width - len(o)) for o in out], dtype=torch.long, device=dev)
    return ids if n_return is None else (ids, torch.tensor(out_scores, dtype=torch.float32, device=dev))


def contrastive_search(step, reorder_cache, ids, ml, am, pixel_values, visual_features, max_length, contrastive, eos, pad, processors=None,
                       logprob_dtype=None, constraints=None, trace=None):
    """Contrastive search (rules T, C1 - C7 of include/flamingo_fusion.h) over the cached decode path with growing caches; `step` is
    FlamingoModel._contrastive_step - (last logits (rows, V) float, lm_head inputs (rows, positions, dim), past) -, `reorder_cache`
    FlamingoModel._reorder_cache, `contrastive` a Contrastive.  The prompt runs once per sequence and gives H[:, :L0] and the first
    candidates; every later step feeds the k candidates of every sequence (the caches expanded b -> b k by reorder_cache with a repeated
    index), ranks them with contrastive_select_torch, appends the chosen token and its lm_head input, and selects the chosen rows back
    (reorder_cache with sel_row).  Processors and constraints act on the chosen row's logits before the next candidates are listed; the eos
    bookkeeping is dynamic_decode's.  It also runs on CPU tensors.  With `logprob_dtype` it returns (ids, token_logprobs): logp of the chosen
    candidate, 0 for a row that had finished.  `trace` (a list) receives one dict per step: what the selection read and what it chose."""
    b, L0 = ids.shape
    k, alpha = contrastive.k, contrastive.penalty_alpha
    fill = pad if pad is not None else 0
    dev = ids.device
    process = _dynamic_processor(processors, eos, L0, constraints)
    finished = torch.zeros(b, dtype=torch.bool, device=dev)
    lps = []
    logits, hidden, past = step(ids, ml, am, None, pixel_values, visual_features)
    hist, mask = hidden, am != 0                                          # (b, n, dim), (b, n)
    x = process(logits if logprob_dtype is None else logits.to(logprob_dtype), ids)
    cand_tok, cand_logp = topk_logprobs_torch(x, k)
    expand = torch.arange(b, device=dev).repeat_interleave(k)
    while ids.shape[1] < max_length:
        ml = torch.cat([ml, torch.zeros_like(ml[:, :1])], dim=1)
        am = torch.cat([am, torch.ones_like(am[:, :1])], dim=1)
        logits, hidden, past = step(cand_tok.reshape(-1, 1).to(ids.dtype), _repeat_leading(ml, k), _repeat_leading(am, k), reorder_cache(past, expand), None, None)
        h = hidden[:, -1]                                                 # (b k, dim)
        nxt, lp, c, done, score = contrastive_select_torch(h, hist, mask, cand_tok, cand_logp, finished, alpha, eos, fill)
        sel_row = torch.arange(b, device=dev) * k + c
        if trace is not None:
            trace.append(dict(x=x, hidden=h, hist=hist, mask=mask, cand_tok=cand_tok, cand_logp=cand_logp, finished=finished, next_tok=nxt, logprob=lp,
                              sel_row=sel_row, score=score))
        lps.append(lp)
        finished = done
        hist = torch.cat([hist, h.index_select(0, sel_row)[:, None]], dim=1)
        mask = torch.cat([mask, torch.ones_like(mask[:, :1])], dim=1)
        ids = torch.cat([ids, nxt[:, None].to(ids.dtype)], dim=1)
        if ids.shape[1] >= max_length or (eos is not None and bool(finished.all())):
            break
        past = reorder_cache(past, sel_row)
        nl = logits.index_select(0, sel_row)
        x = process(nl if logprob_dtype is None else nl.to(logprob_dtype), ids)
        cand_tok, cand_logp = topk_logprobs_torch(x, k)
    if logprob_dtype is not None:
        return ids, (torch.stack(lps, dim=1).to(logprob_dtype) if lps else torch.zeros((b, 0), dtype=logprob_dtype, device=dev))
    return ids


# ---- exact closed-set scoring: the candidate trie walked level by level (FlamingoModel.score_candidates) ----
@dataclasses.dataclass
class CandidateScores:
    """What score_candidates() returns.  `logprobs` (b, k), float32 (float64 for a model that computes in float64): for sequence s and
    candidate j, in the caller's order, sum_t log p(c_j[t] | media_s, prompt_s, c_j[:t]), plus log p(eos | media_s, prompt_s, c_j) when eos
    is scored.  `token_counts` (k,) int64: the number of scored tokens, eos included when it is scored."""
    logprobs: torch.Tensor
    token_counts: torch.Tensor


def logprob_gather_torch(logits, row_first, tok, base=None):
    """Rules S1 - S3 of ff_logprob_gather (include/flamingo_fusion.h) restated in torch, on tensors of any device: out[q] = (base[r] +)
    log_softmax(logits[r])[tok[q]] for the queries q in [row_first[r], row_first[r + 1]) of row r, bounds clamped into [0, n_q].  The math
    is float32, float64 for float64 logits, and so is the result; a token outside [0, V) gives NaN, -inf at the token -inf, a row holding
    NaN or +inf NaN; only rows with a non-empty list are read, and a query no row owns stays NaN."""
    rows, V = logits.shape
    n_q = tok.numel()
    dt = torch.float64 if logits.dtype == torch.float64 else torch.float32
    dev = logits.device
    out = torch.full((n_q,), float("nan"), dtype=dt, device=dev)
    rf = row_first.to(torch.long).clamp(0, n_q)
    counts = (rf[1:] - rf[:-1]).clamp(min=0)
    total = int(counts.sum())
    if total == 0:
        return out
    row_of = torch.repeat_interleave(torch.arange(rows, device=dev), counts)
    q = rf[:-1][row_of] + torch.arange(total, device=dev) - (counts.cumsum(0) - counts)[row_of]
    used = (counts > 0).nonzero()[:, 0]
    x = logits.index_select(0, used).to(dt)                                 # rows without queries are not read
    lse = torch.logsumexp(x, dim=-1)
    lse = torch.where(torch.isnan(lse) | (lse == float("inf")), torch.full_like(lse, float("nan")), lse)
    slot = torch.zeros(rows, dtype=torch.long, device=dev)
    slot[used] = torch.arange(used.numel(), device=dev)
    t = tok.to(torch.long)[q]
    valid = (t >= 0) & (t < V)
    lp = x[slot[row_of], t.clamp(0, V - 1)] - lse[slot[row_of]]
    lp = torch.where(valid, lp, torch.full_like(lp, float("nan")))
    if base is not None:
        lp = base.to(dt)[row_of] + lp
    out[q] = lp
    return out


def _ranges(starts, counts):
    """numpy: the concatenation of arange(starts[i], starts[i] + counts[i])"""
    import numpy as np
    return np.repeat(starts - (np.cumsum(counts) - counts), counts) + np.arange(int(counts.sum()))


def trie_levels(trie, eos, b, max_rows):
    """The host-side tables of score_trie, built once per call from the TokenTrie arrays with numpy.  A node NEEDS LOGITS when it has an
    edge, or when it is terminal and eos is scored.  The root's subtrees are split, in edge order, into groups in which the widest level
    (nodes needing logits) times b stays within max_rows; a single subtree wider than that forms a group alone.  Returns a list of groups,
    each a list of levels (depth 0 = the root, restricted to the group's edges), each level a dict:
    `R` nodes / rows per sequence, `Q` queries per sequence, `row_first` (b R + 1,) and `tok` (b Q,) int32, sequence-major - a node's
    queries are its edge tokens, then eos if it is terminal and eos is scored -; `fin_q` / `fin_nodes`: the queries whose result is the
    finished score of a terminal node; `next_q` / `next_parent` / `next_tok`: the queries that open a row of the next level, the row (within
    the sequence) they hang from and the token to feed."""
    import numpy as np
    nf, et, ec = trie.node_first.astype(np.int64), trie.edge_tok.astype(np.int64), trie.edge_child.astype(np.int64)
    term = trie.node_terminal.astype(bool)
    N, deg = trie.n_nodes, np.diff(trie.node_first.astype(np.int64))
    eos_on = eos is not None
    needs = (deg > 0) | (term & eos_on)
    edge_parent = np.repeat(np.arange(N), deg)
    depth, sub = np.zeros(N, np.int64), np.full(N, -1, np.int64)        # sub: the root edge a node descends from
    frontier, d = np.array([0]), 0
    while frontier.size:
        e = _ranges(nf[frontier], deg[frontier])
        depth[ec[e]] = d + 1
        sub[ec[e]] = e if d == 0 else sub[edge_parent[e]]
        frontier, d = ec[e], d + 1
    n_sub = int(deg[0])
    width = np.zeros((n_sub, int(depth.max()) + 1), np.int64)
    inner = np.flatnonzero(needs[1:]) + 1
    np.add.at(width, (sub[inner], depth[inner]), 1)
    bounds, cur = [0], np.zeros(width.shape[1], np.int64)
    for s in range(n_sub):
        if s > bounds[-1] and int((cur + width[s]).max()) * b > max_rows:
            bounds.append(s)
            cur = np.zeros_like(cur)
        cur = cur + width[s]
    bounds.append(n_sub)
    groups = []
    for lo, hi in zip(bounds[:-1], bounds[1:]):
        levels, nodes = [], np.array([0])
        while nodes.size:
            R = nodes.size
            starts, counts = (np.array([lo]), np.array([hi - lo])) if not levels else (nf[nodes], deg[nodes])
            has_eos = term[nodes] & eos_on
            cnt = counts + has_eos
            first = np.cumsum(cnt) - cnt
            Q = int(cnt.sum())
            e, qe = _ranges(starts, counts), _ranges(first, counts)
            tok = np.empty(Q, np.int64)
            tok[qe] = et[e]
            if eos_on:
                tok[(first + counts)[has_eos]] = eos
            children = ec[e]
            fin = term[children] & (not eos_on)
            opens = needs[children]
            levels.append(dict(R=R, Q=Q, tok=np.tile(tok, b).astype(np.int32),
                               row_first=np.concatenate([[0], np.cumsum(np.tile(cnt, b))]).astype(np.int32),
                               fin_q=(first + counts)[has_eos] if eos_on else qe[fin], fin_nodes=nodes[has_eos] if eos_on else children[fin],
                               next_q=qe[opens], next_parent=np.repeat(np.arange(R), counts)[opens], next_tok=et[e][opens]))
            nodes = children[opens]
        groups.append(levels)
    return groups


def score_trie(step, reorder_cache, ids, ml, am, pixel_values, visual_features, candidate_ids, vocab, eos=None, max_rows=1024):
    """Exact log p(candidate | media, prompt) of every candidate for every sequence, each distinct candidate prefix run once: the candidate
    trie (TokenTrie) walked level-synchronously over the cached decode path.  `step(step_ids, ml, am, past, pixel_values, visual_features)`
    returns (the last position's logits (rows, V) - in the model's dtype, a view is fine -, past), `reorder_cache(past, idx)` gathers cache
    rows (idx may be longer than the cache has rows): FlamingoModel._score_step / ._reorder_cache.
    The prompt step runs on the b rows; its logits are the root's.  At depth d the rows are (sequence, node needing logits at depth d),
    sequence-major, a sequence's nodes in lexicographic order of their prefixes; ONE logprob_gather serves the level - functional.logprob_gather (ff_logprob_gather, the logits read in place in their
    dtype, no (rows, V) float32 temporary) on GPU tensors, logprob_gather_torch on CPU tensors -, with the path's accumulated score as
    `base`, and its result splits into the next level's bases and the finished scores.  The next level is one LM step on the edge tokens,
    the caches gathered from the parent rows; media_locations gains a zero column, the attention mask a one column.  After the prompt that
    is longest - 1 steps, longest when eos is scored.
    `max_rows` bounds memory: the root's subtrees are split, in edge order, into groups whose widest level times b stays within it (a
    single subtree wider than that runs alone, over the bound), and each group is walked on its own.  For every group the b-row prompt step
    is RE-RUN (the caches of a group are gathered in place, and a prompt step of b rows costs less than a deep copy of its caches is worth
    keeping); pass `visual_features`, not pixel_values, so that the visuals are not encoded again (score_candidates does).
    This is the dynamic path: the row count changes with every level, nothing is captured into a graph.
    ValueError: what TokenTrie raises for the candidates; max_rows not an int >= 1."""
    import numpy as np
    if isinstance(max_rows, bool) or not isinstance(max_rows, int) or max_rows < 1:
        raise ValueError(f"score_candidates(): max_rows must be an integer >= 1, got {max_rows!r}")
    if eos is not None and (isinstance(eos, bool) or not isinstance(eos, int) or not 0 <= eos < vocab):
        raise ValueError(f"score_candidates(): eos_token_id must be a token id in [0, {vocab}), got {eos!r}")
    if hasattr(candidate_ids, "__iter__") and not isinstance(candidate_ids, (str, bytes)):
        candidate_ids = list(candidate_ids)                            # (read twice: by the trie, and for the columns)
    trie = TokenTrie(candidate_ids, vocab, eos)
    b, dev = ids.shape[0], ids.device
    child = dict(zip(zip(np.repeat(np.arange(trie.n_nodes), np.diff(trie.node_first)).tolist(), trie.edge_tok.tolist()), trie.edge_child.tolist()))
    columns = []                                                       # caller column -> terminal node (duplicates share one)
    for c in candidate_ids:
        s = 0
        for t in c:
            s = child[(s, int(t))]
        columns.append(s)
    dev_idx = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    node_scores = None
    for levels in trie_levels(trie, eos, b, max_rows):
        logits, past = step(ids, ml, am, None, pixel_values, visual_features)
        ml_g, am_g, base = ml, am, None
        for lv in levels:
            gather = F.logprob_gather if logits.is_cuda else logprob_gather_torch
            out = gather(logits, dev_idx(lv["row_first"]), dev_idx(lv["tok"]), base).view(b, lv["Q"])
            if node_scores is None:
                node_scores = torch.full((b, trie.n_nodes), float("nan"), dtype=out.dtype, device=dev)
            if lv["fin_q"].size:
                node_scores[:, dev_idx(lv["fin_nodes"])] = out[:, dev_idx(lv["fin_q"])]
            if not lv["next_q"].size:
                break
            rows_from = dev_idx((np.arange(b)[:, None] * lv["R"] + lv["next_parent"][None, :]).reshape(-1))
            base = out[:, dev_idx(lv["next_q"])].reshape(-1)
            past = reorder_cache(past, rows_from)
            ml_g = torch.cat([ml_g.index_select(0, rows_from), torch.zeros_like(ml_g[:1, :1]).expand(rows_from.numel(), 1)], dim=1)
            am_g = torch.cat([am_g.index_select(0, rows_from), torch.ones_like(am_g[:1, :1]).expand(rows_from.numel(), 1)], dim=1)
            step_ids = dev_idx(np.tile(lv["next_tok"], b)).to(ids.dtype)[:, None]
            logits, past = step(step_ids, ml_g, am_g, past, None, None)
    counts = torch.tensor([len(c) + (eos is not None) for c in candidate_ids], dtype=torch.long, device=dev)
    return CandidateScores(logprobs=node_scores[:, dev_idx(np.array(columns, np.int64))], token_counts=counts)
