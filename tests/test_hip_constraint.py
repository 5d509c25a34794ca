"""Constrained decoding on the graph-replayed decode path, on the GPU: ff_logits_constrain (functional.constrain_logits,
csrc/ff_constrain.hip) against the numpy restatement of its rules (tests/constraint_cases.py) BIT FOR BIT over the whole rows x ld buffer on
the designed cases, under graph replay with device-side tables, history and lengths, and inside the greedy, sampling and beam _DecodeSession
of FlamingoModel.generate(candidate_ids=, bad_words_ids=).

Nothing here has a tolerance of its own: the rules write -inf and everything else keeps its bits.  In the session tests a step is
undecidable only when the two largest restated logits are exactly equal (greedy), under the EDGE rule of tests/test_hip_sampling.py
(sampling) or the margin rule of tests/test_hip_beam.py (beams); at most 5 % of the steps may be.  Log-probabilities are held to the loss
bound of tests/test_hip_logprob.py against float64 over the restated row."""
import contextlib

import numpy as np
import pytest
import torch

import beam_cases as BC
import constraint_cases as CC

BF16, F32 = torch.bfloat16, torch.float32
TORCH = {"bf16": (BF16, torch.int16, np.int16, np.uint16(0x7FA5)), "f32": (F32, torch.int32, np.int32, np.uint32(0x7FA5A5A5))}
TRIE_KEYS = ("node_first", "edge_tok", "edge_child", "node_terminal", "n_nodes")
WORD_KEYS = ("bw_off", "bw_tok", "n_bw")


def device_tables(t, keys):
    """the table's arrays on the device, in the order functional.constrain_logits takes them (the live size as a one-element int32 tensor)"""
    return tuple(torch.from_numpy(np.atleast_1d(np.asarray(t[k], np.int32 if k.startswith("n_") else t[k].dtype))).cuda() for k in keys)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", CC.SHAPES, ids=lambda s: f"{s[0]}x{s[1]}-{s[2]}")
def test_kernel_equals_the_restatement_bit_for_bit(shape):
    """Every (hist_cap, *hist_len, *gen_start) of LENGTHS x {trie and words, trie, words}: the WHOLE buffer equals the restatement's bits.
    Even cases are contiguous rows (ld == V), odd ones the view buf[:, 1:1 + V] of rows 11 elements wider (a base offset of one element, a
    different misalignment in every row, poisoned gaps); the buffer comes from the guarded allocation seam (guards before and after it);
    the tables sit in arrays of twice their live size with garbage behind; odd cases pass the history as a view with hist_ld > hist_cap."""
    from guarded import guarded_allocations
    from flamingo_mini_amd import functional as F
    rows, V, dtype = shape
    tdt, idt, ndt, poison = TORCH[dtype]
    eos = CC.EOS
    trie, _ = CC.trie_for(V, eos)
    trie_dev = device_tables(CC.pad_tables(trie, V), TRIE_KEYS)
    hist_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    gen_start_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    rng = np.random.default_rng(V + rows)
    bad, launches, moved, live = [], 0, 0, 0
    with guarded_allocations() as guards:
        bufs = {0: F._new((rows, V), tdt, "cuda"), 1: F._new((rows, V + 11), tdt, "cuda")}
        for k, (cap, n, n0, rot) in enumerate(CC.LENGTHS):
            nn, nn0 = CC.clamped(cap, n, n0)
            hist = CC.histories(V, eos, rows, cap, nn, nn0, rng, rot)
            words = CC.words_for(V, hist, nn)
            words_dev = device_tables(CC.pad_tables(words, k), WORD_KEYS)
            hist_dev = torch.from_numpy(hist).cuda()
            if k % 2:
                big = torch.zeros((rows, cap + 3), dtype=torch.long, device="cuda")
                big[:, :cap] = hist_dev
                hist_dev = big[:, :cap]
            hist_len_dev.fill_(n)
            gen_start_dev.fill_(n0)
            for which in ("both", "trie", "words"):
                buf, off = bufs[k % 2], k % 2
                bits = CC.make_logits(rows, V, dtype, 100 * k + len(which))
                full = np.full(tuple(buf.shape), poison, bits.dtype)
                full[:, off:off + V] = bits
                buf.view(idt).copy_(torch.from_numpy(full.view(ndt)).cuda())
                view = buf[:, off:off + V]
                out = F.constrain_logits(view, hist_dev, hist_len_dev, gen_start_dev, eos if which != "words" else None,
                                         trie=trie_dev if which != "words" else None, bad_words=words_dev if which != "trie" else None)
                assert out is view
                got = buf.view(idt).cpu().numpy().view(bits.dtype)
                want = full.copy()
                want[:, off:off + V] = CC.restate(bits, V, hist, n, n0, eos=eos, trie=trie if which != "words" else None,
                                                  words=words if which != "trie" else None, dtype=dtype)
                launches += 1
                if not np.array_equal(got, want):
                    r, c = np.argwhere(got != want)[0]
                    bad.append((cap, n, n0, which, int(r), int(c) - off, hex(int(got[r, c])), hex(int(want[r, c])), int((got != want).sum())))
                moved += not np.array_equal(want, full)
                if which == "trie":                                           # rows the trie rule masks, and rows it leaves alone
                    changed = (want != full).any(1)
                    live += int(changed.sum())
        guards.check()
    assert not bad, f"{len(bad)} of {launches} (cap, n, n0, tables, row, column, got, want, count): {bad[:6]}"
    assert moved >= launches * 3 // 4 and live >= len(CC.LENGTHS), (moved, launches, live)


@pytest.mark.gpu
def test_replay_follows_device_side_tables_history_and_lengths():
    """captured once; then the tables (other candidates and words, in the same buffers), the history, *hist_len and *gen_start change on the
    device and the replay follows them"""
    from flamingo_mini_amd import functional as F
    rows, V, cap, dtype, eos = 3, 320, 96, "bf16", CC.EOS
    tdt, idt, ndt, _ = TORCH[dtype]
    buf = torch.zeros((rows, V), dtype=tdt, device="cuda")
    hist_dev = torch.zeros((rows, cap), dtype=torch.long, device="cuda")
    hist_len_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    gen_start_dev = torch.zeros(1, dtype=torch.long, device="cuda")
    i32 = lambda n, dt=torch.int32: torch.zeros(n, dtype=dt, device="cuda")
    trie_dev = (i32(1025), i32(1024), i32(1024), i32(1024, torch.uint8), i32(1))
    words_dev = (i32(17), i32(64), i32(1))
    call = lambda: F.constrain_logits(buf, hist_dev, hist_len_dev, gen_start_dev, eos, trie=trie_dev, bad_words=words_dev)
    call()                                                                    # (n_nodes == 0, n_bw == 0: nothing moves)
    graph = torch.cuda.CUDAGraph()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph):
        call()
    rng = np.random.default_rng(5)
    sets = [(CC.trie_for(V, eos)[0], 3, 5), (CC.build_trie([[0, 5], [7, 6, 7], [V - 1]]), 3, 4), (CC.build_trie([[0, 1, 2, 3, 4, 5, 6, 7, 8]]), 0, 4),
            (dict(CC.build_trie([[2]]), n_nodes=0), 3, 5)]
    seen = []
    for trie, n0, n in sets:
        hist = CC.histories(V, eos, rows, cap, n, n0, rng)
        if n0 == 0:
            hist[:, :4] = [0, 1, 2, 3]
        words = CC.build_words([[int(hist[1, n - 1]), 40], [41]] if len(seen) % 2 == 0 else [])
        for dev, t, keys in ((trie_dev, trie, TRIE_KEYS), (words_dev, words, WORD_KEYS)):
            for d, k in zip(dev, keys):
                a = np.atleast_1d(np.asarray(t[k], np.int32 if k.startswith("n_") else t[k].dtype))
                d.fill_(77)                                                   # what lies behind the live entries is not read
                d[:len(a)].copy_(torch.from_numpy(a).cuda())
        bits = CC.make_logits(rows, V, dtype, 7 + len(seen))
        buf.view(idt).copy_(torch.from_numpy(bits.view(ndt)).cuda())
        hist_dev.copy_(torch.from_numpy(hist).cuda())
        hist_len_dev.fill_(n)
        gen_start_dev.fill_(n0)
        graph.replay()
        want = CC.restate(bits, V, hist, n, n0, eos=eos, trie=trie, words=words, dtype=dtype)
        assert np.array_equal(buf.view(idt).cpu().numpy().view(bits.dtype), want), len(seen)
        seen.append(int((want != bits).sum()))
    assert seen[0] > 0 and seen[1] > 0 and seen[2] > 0 and seen[3] == 0 and len(set(seen)) == 4, seen


# ---------------------------------------------------------------------------------------------------------------------------------------
# the decode sessions (G1 geometry of tests/test_hip_decode.py, batch 4)
# ---------------------------------------------------------------------------------------------------------------------------------------
TAG = "constraint"
EOS, PAD = 301, 0
CANDS = [[17], [23, 41], [23, 41, 7], [5, 6, 7, 8], [90, 91, 92, 93, 94], [150, 3, 150]]     # 1 - 5 tokens; (23, 41) is a prefix of (23, 41, 7)
OTHER = [[200], [201, 202], [201, 203, 204], [17, 18], [250, 251, 252, 253, 254], [9]]       # the same capacity class, no candidate in common
CKW = dict(candidate_ids=CANDS, eos_token_id=EOS, pad_token_id=PAD)


@pytest.fixture(scope="module")
def g1():
    import test_hip_decode as D
    model, _ = D.models("gpt2")
    inputs = D.make_inputs(4, 1, TAG)
    model.reset_decode_sessions()
    dtype = {BF16: "bf16", F32: "f32"}[next(model.parameters()).dtype]
    yield D, model, inputs, dtype
    model.decode_graph = True
    model.reset_decode_sessions()
    D._MODELS.clear()


def generate(model, inputs, max_length, graph=True, rec=None, **kw):
    ids, ml, am, vf = inputs
    model.decode_graph = graph
    try:
        with (rec.installed() if rec is not None else contextlib.nullcontext()):
            return model.generate(ids, media_locations=ml, attention_mask=am, visual_features=vf, max_length=max_length, **kw)
    finally:
        model.decode_graph = True


def restated(raw, dtype, hist, L0, cands=None, words=None):
    return CC.restate_values(raw, dtype, hist, L0, eos=EOS, trie=CC.build_trie(cands) if cands else None, words=CC.build_words(words) if words else None)


def candidates_of(ids, L0, cands, pad=PAD):
    """every row is prompt + candidate + eos + pad...: the candidates, row by row"""
    found = []
    for row in ids[:, L0:].tolist():
        assert EOS in row, row
        k = row.index(EOS)
        assert row[:k] in cands and all(t == pad for t in row[k + 1:]), row
        found.append(row[:k])
    return found


def greedy_steps_follow(raw, ids, dtype, L0, cands):
    undecidable, bad, total = 0, [], 0
    alive = np.ones(ids.shape[0], bool)
    for pos in range(L0, ids.shape[1]):
        x = restated(raw[:, pos], dtype, ids[:, :pos], L0, cands)
        for r in np.flatnonzero(alive):
            total += 1
            top = np.sort(x[r])[-2:]
            if top[0] == top[1]:
                undecidable += 1
            elif int(np.argmax(x[r])) != ids[r, pos]:
                bad.append((int(r), pos, int(ids[r, pos]), int(np.argmax(x[r]))))
        alive &= ids[:, pos] != EOS
    return undecidable, bad, total


@pytest.mark.gpu
def test_greedy_session_generates_only_candidates_step_for_step(g1):
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, dtype = g1
    plain = generate(model, inputs, D.MAXLEN)
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, **CKW)
    sess = rec.session
    key = [k for k, s in model._decode_sessions.items() if s is sess][0]
    assert sess.constraints == key[-1] == ("constraints", 64, 64, 0, 0) and len(key) == 11 and sess.processors is None
    assert sess.replay is not None and not sess.capture_failed and int(sess.gen_start) == D.L0 and int(sess.trie_bufs[4]) == CC.build_trie(CANDS)["n_nodes"]
    assert torch.equal(out[:, :D.L0], inputs[0]) and not torch.equal(out, plain[:, :out.shape[1]])
    candidates_of(out, D.L0, CANDS)
    undecidable, bad, total = greedy_steps_follow(sess._rec.clone().cpu().numpy(), out.cpu().numpy(), dtype, D.L0, CANDS)
    print(f"MEASURED greedy-under-a-trie undecidable {undecidable} of {total}")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total
    assert torch.equal(out, generate(model, inputs, D.MAXLEN, graph=False, **CKW))
    # other candidates of the same capacity class: the same session object, the same captured graph, the new set obeyed
    graph_before = sess.graph
    rec2 = _SampleRecorder()
    out2 = generate(model, inputs, D.MAXLEN, rec=rec2, **dict(CKW, candidate_ids=OTHER))
    assert rec2.session is sess and sess.graph is graph_before and sess.replay is not None
    candidates_of(out2, D.L0, OTHER)
    undecidable, bad, total = greedy_steps_follow(sess._rec.clone().cpu().numpy(), out2.cpu().numpy(), dtype, D.L0, OTHER)
    assert not bad and undecidable <= 0.05 * total, bad[:8]
    candidates_of(generate(model, inputs, D.MAXLEN, static_decode=False, **dict(CKW, candidate_ids=OTHER)), D.L0, OTHER)   # the dynamic loop's torch restatement


@pytest.mark.gpu
def test_sampling_session_draws_from_the_constrained_logits(g1):
    """the float64 reference of tests/test_hip_sampling.py on the restatement's output and the session's own random numbers, under its EDGE rule"""
    from test_hip_sampling import EDGE, SAMPLING, Ref, _SampleRecorder
    D, model, inputs, dtype = g1
    kw = dict(SAMPLING, do_sample=True, static_decode=True, **CKW)
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    sess = rec.session
    assert sess.sampling == (0.8, 20, 0.9) and sess.constraints is not None and sess.replay is not None and not sess.capture_failed
    found = candidates_of(out, D.L0, CANDS)
    raw, u_all, ids = sess._rec.clone().cpu().numpy(), sess.u_all.clone().cpu().numpy(), out.cpu().numpy()
    T, k, p = sess.sampling
    undecidable, bad, total = 0, [], 0
    alive = np.ones(4, bool)
    for pos in range(D.L0, ids.shape[1]):
        x = restated(raw[:, pos], dtype, ids[:, :pos], D.L0, CANDS).astype(np.float64)
        for r in np.flatnonzero(alive):
            total += 1
            ref = Ref(x[r], T, k)
            P, _, c = ref.cdf(p)
            u = float(u_all[pos, r])
            if np.abs(np.concatenate([[0.0], c[P]]) - u).min() < EDGE or np.abs(ref.above - p).min() < EDGE:
                undecidable += 1
            elif ref.token(p, u) != ids[r, pos]:
                bad.append((int(r), pos, int(ids[r, pos]), ref.token(p, u)))
        alive &= ids[:, pos] != EOS
    print(f"MEASURED sampling-under-a-trie undecidable {undecidable} of {total}; drew {found}")
    assert not bad, f"(row, position, got, want): {bad[:8]}"
    assert undecidable <= 0.05 * total
    eager = generate(model, inputs, D.MAXLEN, graph=False, generator=torch.Generator(device="cuda").manual_seed(1), **kw)
    assert torch.equal(eager, out)


@pytest.mark.gpu
def test_beam_session_keeps_every_beam_inside_the_trie(g1):
    """3 beams.  The histories are rebuilt from hist_parent; every decidable step's chosen (token, parent) lists of a sequence that is not
    done equal beam_cases.candidates on the RESTATED logits (float64, the margin rule of tests/test_hip_beam.py); the returned ids are
    _beam_finalize of the beam restatement driven by the restated logits; seq_buf followed the beams; eager equals replayed;
    num_return_sequences = 3 returns distinct candidates, scores descending."""
    from flamingo_mini_amd.modeling_flamingo import _beam_finalize
    from test_hip_beam import NB, SCORE_BOUND, beam_generate, gaps_decidable
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, dtype = g1
    rec = _SampleRecorder()
    res = beam_generate(model, inputs, D.MAXLEN, rec=rec, num_return_sequences=NB, return_dict_in_generate=True, **CKW)
    out = res.sequences
    sess = rec.session
    assert sess.beams == (NB, True, 1.0) and sess.processors is None and sess.constraints is not None and sess.seq_buf.shape == (4 * NB, D.MAXLEN)
    assert sess.replay is not None and not sess.capture_failed
    raw, host = sess._rec.clone().cpu().numpy(), sess.state.to_host()
    assert not np.isnan(host["hist_score"][D.L0:D.MAXLEN]).any() and not np.isnan(host["score"]).any() and not np.isnan(host["hyp_score"][host["hyp_len"] > 0]).any()
    hist = np.repeat(inputs[0].cpu().numpy(), NB, axis=0)
    st = BC.new_state(4, NB, sess.max_length, 1.0, sess.fill)
    undecidable, bad, worst, total = 0, [], 0.0, 0
    for pos in range(D.L0, D.MAXLEN):
        x = restated(raw[:, pos], dtype, hist, D.L0, CANDS)
        assert not np.isnan(x).any()
        prev = BC.new_state(4, NB, 1)["score"] if pos == D.L0 else host["hist_score"][pos - 1].reshape(4, NB)
        top_s, top_b, top_t = BC.candidates(prev, x, NB, np.float64)
        ok, _ = gaps_decidable(top_s, top_b)
        for s in range(4):
            if st["done"][s]:
                continue
            total += 1
            r = slice(s * NB, (s + 1) * NB)
            fin = np.isfinite(host["hist_score"][pos, r])                      # (a dead beam's token is whatever -inf candidate the flat-index rule ranks first)
            got = (host["hist_tok"][pos, r][fin].tolist(), host["hist_parent"][pos, r][fin].tolist())
            want_tp = [(int(t), int(s * NB + b)) for sc, t, b in zip(top_s[s], top_t[s], top_b[s]) if t != EOS and np.isfinite(sc)][:NB]
            if not ok[s]:
                undecidable += 1
            elif got != ([t for t, _ in want_tp], [b for _, b in want_tp]):
                bad.append((s, pos, got, want_tp))
            elif fin.any():
                ref = np.array([sc for sc, t in zip(top_s[s], top_t[s]) if t != EOS and np.isfinite(sc)][:NB])
                worst = max(worst, float(np.abs(host["hist_score"][pos, r][fin].astype(np.float64) - ref).max()))
        BC.step(st, x, pos + 1, NB, EOS, sess.fill, True)
        hist = np.concatenate([hist[host["hist_parent"][pos]], host["hist_tok"][pos][:, None]], axis=1)
    print(f"MEASURED beams-under-a-trie undecidable {undecidable} of {total}; score error {worst:.3e}")
    assert not bad, f"(sequence, position, got, want): {bad[:4]}"
    assert worst <= SCORE_BOUND and undecidable <= 0.05 * total
    assert np.array_equal(sess.seq_buf.cpu().numpy(), hist), "seq_buf did not follow the beams"
    st["length"], st["eos"] = D.MAXLEN, EOS
    want_ids, want_scores = _beam_finalize(st, D.L0, inputs[0].cpu(), NB, sess.fill, n_return=NB)
    assert torch.equal(out.cpu(), want_ids[:, :out.shape[1]]) and bool((want_ids[:, out.shape[1]:] == sess.fill).all())
    found = candidates_of(out, D.L0, CANDS)
    for s in range(4):
        mine, sc = found[NB * s:NB * s + NB], res.sequences_scores[NB * s:NB * s + NB].cpu()
        assert len({tuple(c) for c in mine}) == NB and bool(torch.isfinite(sc).all()) and bool((sc[:-1] >= sc[1:]).all()), (mine, sc)
        assert np.abs(sc.numpy().astype(np.float64) - want_scores[NB * s:NB * s + NB].numpy()).max() <= SCORE_BOUND
    eager = beam_generate(model, inputs, D.MAXLEN, graph=False, num_return_sequences=NB, return_dict_in_generate=True, **CKW)
    assert torch.equal(eager.sequences, out) and torch.equal(eager.sequences_scores, res.sequences_scores)
    assert torch.equal(beam_generate(model, inputs, D.MAXLEN, **CKW), out[::NB][:, :max(len(c) for c in found[::NB]) + D.L0 + 1])


@pytest.mark.gpu
def test_two_candidates_and_three_beams(g1):
    """fewer candidates than beams: both come back, best first, the third row is all pad with score -inf, and no score of any step is NaN"""
    from test_hip_beam import NB, beam_generate
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, _ = g1
    two = [[23, 41], [5, 6, 7, 8]]
    rec = _SampleRecorder()
    res = beam_generate(model, inputs, D.MAXLEN, rec=rec, num_return_sequences=NB, return_dict_in_generate=True, **dict(CKW, candidate_ids=two))
    host = rec.session.state.to_host()
    assert rec.session.replay is not None
    assert not np.isnan(host["hist_score"][D.L0:D.MAXLEN]).any() and not np.isnan(host["score"]).any(), "a NaN score"
    rows, sc = res.sequences[:, D.L0:].cpu().tolist(), res.sequences_scores.cpu()
    for s in range(4):
        a, b, c = rows[NB * s:NB * s + NB]
        assert sorted([a[:a.index(EOS)], b[:b.index(EOS)]]) == sorted(two) and all(t == PAD for t in c), (a, b, c)
        assert bool(torch.isfinite(sc[NB * s:NB * s + 2]).all()) and float(sc[NB * s]) >= float(sc[NB * s + 1]) and float(sc[NB * s + 2]) == -np.inf


@pytest.mark.gpu
def test_log_probabilities_under_a_trie_are_renormalised_over_the_allowed_set(g1):
    """output_logprobs=True: every value is within the loss bound (tests/util.py CE_C_F) of float64 log-softmax over the RESTATED row built
    from the recorded raw logits; exactly 0 after eos; the eos token carries its own (0 at a leaf, where eos is the only token allowed)"""
    import logprob_cases as LP
    from test_hip_sampling import _SampleRecorder
    from util import CE_C_F
    D, model, inputs, dtype = g1
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, static_decode=True, return_dict_in_generate=True, output_logprobs=True, **CKW)
    sess = rec.session
    assert sess.logprobs and sess.constraints is not None and sess.replay is not None and not sess.capture_failed
    raw, ids, lps = sess._rec.clone().cpu().numpy(), out.sequences.cpu().numpy(), out.token_logprobs.cpu()
    found = candidates_of(out.sequences, D.L0, CANDS)
    finished = np.zeros(4, bool)
    worst, leaves = 0.0, 0
    for pos in range(D.L0, ids.shape[1]):
        x = torch.from_numpy(restated(raw[:, pos], dtype, ids[:, :pos], D.L0, CANDS))
        tok = torch.from_numpy(ids[:, pos])
        if finished.any():
            assert lps[torch.from_numpy(finished), pos - D.L0].view(torch.int32).tolist() == [0] * int(finished.sum())
        live = torch.from_numpy(~finished)
        lp_ref, lse_ref, xt = LP.reference(x[live], tok[live])
        ratio = (lps[live, pos - D.L0].double() - lp_ref).abs() / (CE_C_F * 2.0 ** -24 * (lse_ref.abs() + xt.abs() + 1.0))
        worst = max(worst, float(torch.nan_to_num(ratio, nan=float("inf")).max()))
        for r in np.flatnonzero(~finished):
            if ids[r, pos] == EOS and int(np.isfinite(x[r].numpy()).sum()) == 1:
                assert float(lps[r, pos - D.L0]) == 0.0
                leaves += 1
        finished |= ids[:, pos] == EOS
    print(f"MEASURED log-probabilities under a trie: worst at {worst:.3f} of the bound; {leaves} eos tokens at leaves; chose {found}")
    assert worst <= 1.0
    assert bool((out.token_logprobs <= 0).all()) and bool(torch.isfinite(out.sequences_scores).all())
    eager = generate(model, inputs, D.MAXLEN, graph=False, static_decode=True, return_dict_in_generate=True, output_logprobs=True, **CKW)
    assert torch.equal(eager.sequences, out.sequences) and torch.equal(eager.token_logprobs.view(torch.int32), out.token_logprobs.view(torch.int32))


@pytest.mark.gpu
def test_bad_words_change_the_ids_and_never_appear(g1):
    """the words come from the unconstrained run's own output - row 0's first generated token, row 1's first bigram, and a bigram that
    starts at the last prompt token of row 2 - so the ban changes the ids; no window that ends at a generated position equals a banned
    word; the session is captured; eager steps and the dynamic loop give the same ids"""
    from test_hip_sampling import _SampleRecorder
    D, model, inputs, dtype = g1
    L0 = D.L0
    plain = generate(model, inputs, D.MAXLEN)
    words = [[int(plain[0, L0])], [int(plain[1, L0]), int(plain[1, L0 + 1])], [int(plain[2, L0 - 1]), int(plain[2, L0])]]
    rec = _SampleRecorder()
    out = generate(model, inputs, D.MAXLEN, rec=rec, bad_words_ids=words)
    sess = rec.session
    assert sess.constraints == ("constraints", 0, 0, 16, 64) and sess.trie_bufs is None and sess.replay is not None and not sess.capture_failed
    assert out.shape == plain.shape and all(not torch.equal(out[r], plain[r]) for r in range(3))
    for row in out.cpu().tolist():
        for w in words:
            assert not any(row[i:i + len(w)] == w for i in range(L0 - len(w) + 1, len(row) - len(w) + 1)), (w, row)
    raw, ids = sess._rec.clone().cpu().numpy(), out.cpu().numpy()
    undecidable, bad = 0, []
    for pos in range(L0, ids.shape[1]):
        x = CC.restate_values(raw[:, pos], dtype, ids[:, :pos], L0, words=CC.build_words(words))
        for r in range(4):
            top = np.sort(x[r])[-2:]
            if top[0] == top[1]:
                undecidable += 1
            elif int(np.argmax(x[r])) != ids[r, pos]:
                bad.append((r, pos))
    assert not bad and undecidable <= 0.05 * 4 * (ids.shape[1] - L0), (bad[:8], undecidable)
    assert torch.equal(out, generate(model, inputs, D.MAXLEN, graph=False, bad_words_ids=words))
    both = generate(model, inputs, D.MAXLEN, bad_words_ids=[[17], [23, 41, 7]], **CKW)      # with a trie: the banned candidates are never chosen
    assert not any(c in ([17], [23, 41, 7]) for c in candidates_of(both, L0, CANDS))
