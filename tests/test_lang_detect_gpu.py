"""Whisper's language detection on the device (language = "auto"): k_lang_pick alone against the host loop, tk_mi355x_asr_detect_language and
the transcription entry points against the CPU oracle run with the detected language's prompt, the shared engine's coalescing, the
reference-parameter decode and process_audio, and English-only vocabularies, which detect nothing.

The small multilingual geometry of test_asr_set_language_selects_the_decoder_prompt.  MODEL_SEED and PCM_SEED were searched on the CPU oracle
(model seeds 11 - 13, PCM seeds 0 - 5, the three utterances built as utterances() builds them): this pair makes the rows detect three different
languages (88, 21, 31) with the raw synthetic weights and with their f16-rounded checkpoint alike; the tests assert that at least two differ."""
import threading

import numpy as np
import pytest

import lang_pick_cases as LC
import lang_pick_ref as R
import oracle_lib as O

pytestmark = pytest.mark.gpu

ML = (80, 50, 64, 2, 2, 32, 64, 2, 2, 51865)
MODEL_SEED, PCM_SEED = 13, 3
SOT, TOK0, N_LANG, TRANSLATE, TRANSCRIBE, NOTS = 50258, 50259, 99, 50358, 50359, 50363
STEPS = 4


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def utterances():
    rng = np.random.default_rng(PCM_SEED)
    pcm = np.clip(rng.normal(0, 3000, (3, 16000)), -32768, 32767).astype(np.int16)
    pcm[1, 9000:] = 0                                                        # a shorter utterance
    pcm[2] = (pcm[2] * 0.2).astype(np.int16)                                 # a quiet one
    return pcm


def oracle_world(orc):
    """per utterance, from the oracle alone: the language logits of the <|startoftranscript|> step, the restatement's decision on them, and the
    transcription under the prompt that names that language"""
    pcm = utterances()
    lang_logits = np.stack([orc.transcribe(pcm[b:b + 1], 1, prompt=[SOT])[3][0, TOK0:TOK0 + N_LANG] for b in range(3)])
    ids, _, _ = R.pick(lang_logits, 3, N_LANG, N_LANG, 0, N_LANG, np.zeros(3, np.int32), np.zeros(3, np.int32))
    assert len(set(ids.tolist())) >= 2, ids
    want = {}
    for task in (TRANSCRIBE, TRANSLATE):
        want[task] = [orc.transcribe(pcm[b:b + 1], STEPS, prompt=[SOT, TOK0 + int(ids[b]), task, NOTS]) for b in range(3)]
    return dict(pcm=pcm, lang_logits=lang_logits, ids=ids, want=want)


@pytest.fixture(scope="module")
def world():
    return oracle_world(O.OracleWhisper(O.WhisperHP(*ML), seed=MODEL_SEED))


@pytest.fixture(scope="module")
def checkpoint(tmp_path_factory):
    """the same model as a whisper.cpp ggml checkpoint (f16 weights), which tk_asr_whisper_create opens through the shared registry, and the
    oracle's world on the rounded weights"""
    import ggml_whisper_util as G
    ohp = O.WhisperHP(*ML)
    orc = O.OracleWhisper(ohp, seed=MODEL_SEED)
    T = orc.tensors()
    rounded, file_t = G.checkpoint_tensors(T, ohp)
    orc.set_tensors(rounded)
    vocab = [(" w%d" % i).encode() for i in range(SOT - 1)]                  # the text tokens; eot = 50257
    path = tmp_path_factory.mktemp("lang") / "ggml-multilingual.bin"
    G.write_ggml(path, ohp, T["frontend.mel_filters"], vocab, file_t)
    w = oracle_world(orc)
    w.update(path=str(path), orc=orc, vocab=vocab)
    return w


@pytest.mark.parametrize("rows", [1, 2, 17, 256])
def test_the_kernel_alone_is_bit_identical_to_the_host_loop(gpu, rows):
    n = 0
    for n_lang in LC.N_LANGS:
        for c in LC.cases(n_lang, rows):
            args = (c["logits"], c["rows"], c["cols"], c["tok0"], c["n_lang"], c["auto_row"], c["slot"])
            hid, hpr, hsl = gpu.lang_pick_probe(*args, ld=c["ld"], device=-1)
            did, dpr, dsl = gpu.lang_pick_probe(*args, ld=c["ld"], device=0)
            assert np.array_equal(did, hid) and np.array_equal(dsl, hsl), c["name"]
            assert np.array_equal(bits(dpr), bits(hpr)), (c["name"], np.argwhere(bits(dpr) != bits(hpr))[:4])
            n += 1
    assert n >= len(LC.N_LANGS)


def test_detect_language_decides_on_the_oracles_logits(gpu, world):
    asr = gpu.Asr(hp=gpu.WhisperHP(*ML), seed=MODEL_SEED, max_batch=4)
    ids, probs = asr.detect_language(world["pcm"])
    assert np.array_equal(bits(asr.last_language_logits()), bits(world["lang_logits"]))       # the slice of the <|sot|> step's logits, per row
    assert np.array_equal(ids, world["ids"])
    _, hpr, _ = gpu.lang_pick_probe(world["lang_logits"], 3, N_LANG, 0, N_LANG, np.zeros(3, np.int32), np.zeros(3, np.int32), device=-1)
    assert probs.shape == (3, N_LANG) and np.array_equal(bits(probs), bits(hpr))
    lid, lpr = asr.last_languages()
    assert np.array_equal(lid, ids) and np.array_equal(bits(lpr), bits(probs[np.arange(3), ids]))
    one, p1 = asr.detect_language(world["pcm"][1:2])                                          # a row alone answers what it answers in the batch
    assert one[0] == ids[1] and np.array_equal(bits(p1[0]), bits(probs[1]))
    asr.close()


def test_auto_transcribes_every_row_in_its_own_language(gpu, world):
    pcm, ids, want = world["pcm"], world["ids"], world["want"][TRANSCRIBE]
    asr = gpu.Asr(hp=gpu.WhisperHP(*ML), seed=MODEL_SEED, max_batch=4)
    assert asr.set_language("auto") == 0
    assert asr.prompt_tokens() == [SOT, -1, TRANSCRIBE, NOTS]
    toks, _, enc, lg = asr.transcribe_tokens(pcm, STEPS)
    for b in range(3):
        assert np.array_equal(toks[b], want[b][0][0]) and np.array_equal(bits(lg[b]), bits(want[b][3][0])) and np.array_equal(enc[b], want[b][2][0]), b
    _, probs = asr.detect_language(pcm)
    toks2, _, _, _ = asr.transcribe_tokens(pcm, STEPS)
    assert np.array_equal(toks2, toks)
    lid, lpr = asr.last_languages()
    assert np.array_equal(lid, ids) and np.array_equal(bits(lpr), bits(probs[np.arange(3), ids]))
    # one call may mix rows that detect and rows that are told: row 1 in German
    mixed = np.array([-1, 2, -1], np.int32)
    tm, lm = asr.transcribe_tokens_langs(pcm, STEPS, mixed)
    orc = O.OracleWhisper(O.WhisperHP(*ML), seed=MODEL_SEED)
    wde = orc.transcribe(pcm[1:2], STEPS, prompt=[SOT, TOK0 + 2, TRANSCRIBE, NOTS])
    for b in (0, 2):
        assert np.array_equal(tm[b], want[b][0][0]) and np.array_equal(bits(lm[b]), bits(want[b][3][0]))
    assert np.array_equal(tm[1], wde[0][0]) and np.array_equal(bits(lm[1]), bits(wde[3][0]))
    lid, lpr = asr.last_languages()
    assert lid.tolist() == [ids[0], 2, ids[2]] and lpr[1] == 1.0 and np.array_equal(bits(lpr[[0, 2]]), bits(probs[[0, 2], ids[[0, 2]]]))
    with pytest.raises(gpu.TkError):
        asr.transcribe_tokens_langs(pcm, STEPS, [0, N_LANG, 0])
    # the same library told the detected language by name
    for b in range(3):
        assert asr.set_language(gpu.whisper_lang_code(int(ids[b]))) == 0
        assert asr.prompt_tokens() == [SOT, TOK0 + int(ids[b]), TRANSCRIBE, NOTS]
        tb, _, _, lb = asr.transcribe_tokens(pcm[b:b + 1], STEPS)
        assert np.array_equal(tb[0], toks[b]) and np.array_equal(bits(lb[0]), bits(lg[b]))
        lid, lpr = asr.last_languages()
        assert lid.tolist() == [ids[b]] and lpr.tolist() == [1.0]
    asr.close()


def test_translate_changes_only_the_task_token(gpu, checkpoint):
    pcm, ids = checkpoint["pcm"], checkpoint["ids"]
    for translate, task in ((False, TRANSCRIBE), (True, TRANSLATE)):
        asr = gpu.Asr(model=checkpoint["path"], language="auto", translate=translate)
        assert asr.prompt_tokens() == [SOT, -1, task, NOTS]
        for b in range(3):
            toks, _, _, lg = asr.transcribe_tokens(pcm[b:b + 1], STEPS)
            w = checkpoint["want"][task][b]
            assert np.array_equal(toks[0], w[0][0]) and np.array_equal(bits(lg[0]), bits(w[3][0])), (translate, b)
            assert asr.last_languages()[0].tolist() == [ids[b]]
        asr.close()


def test_contexts_of_one_model_coalesce_their_auto_requests(gpu, checkpoint):
    """several contexts on one checkpoint share one engine: three detect, one is told German; every caller gets what it gets alone"""
    pcm, ids, want = checkpoint["pcm"], checkpoint["ids"], checkpoint["want"][TRANSCRIBE]
    langs = ["auto", "auto", "auto", "de"]
    rows = [0, 1, 2, 1]
    ctx = [gpu.Asr(model=checkpoint["path"], language=l) for l in langs]
    wde = checkpoint["orc"].transcribe(pcm[1:2], STEPS, prompt=[SOT, TOK0 + 2, TRANSCRIBE, NOTS])[0][0]
    solo = [ctx[i].transcribe_tokens(pcm[rows[i]:rows[i] + 1], STEPS, want_aux=False)[0][0] for i in range(4)]
    for i in range(3):
        assert np.array_equal(solo[i], want[i][0][0]), i
    assert np.array_equal(solo[3], wde)
    before = ctx[0].share_stats()
    got, seen = [None] * 4, [None] * 4
    bar = threading.Barrier(4)

    def run(i):
        bar.wait()
        got[i] = ctx[i].transcribe_tokens(pcm[rows[i]:rows[i] + 1], STEPS, want_aux=False)[0][0]
        seen[i] = ctx[i].last_languages()

    th = [threading.Thread(target=run, args=(i,)) for i in range(4)]
    for t in th:
        t.start()
    for t in th:
        t.join()
    for i in range(4):
        assert np.array_equal(got[i], solo[i]), i
        assert seen[i][0].tolist() == [ids[i] if i < 3 else 2] and (i < 3 or seen[i][1].tolist() == [1.0])
    after = ctx[0].share_stats()
    assert after[0] == 4 and after[2] - before[2] == 4
    assert after[1] - before[1] < 4 and after[3] >= 2                       # fewer jobs than requests: only the detecting ones share a prompt
    for a in ctx:
        a.close()


def test_the_reference_decode_and_process_audio_follow_the_detected_language(gpu, checkpoint):
    pcm, ids = checkpoint["pcm"], checkpoint["ids"]
    auto, told = gpu.Asr(model=checkpoint["path"], language="auto"), gpu.Asr(model=checkpoint["path"])
    tab, beg, eot = auto.suppress_table()
    assert tab is not None and (beg, eot) == (NOTS + 1, SOT - 1)
    for a in (auto, told):
        a.set_decode_steps(8)
    texts = set()
    for b in range(3):
        assert told.set_language(gpu.whisper_lang_code(int(ids[b]))) == 0
        ga, gt = auto.transcribe_ref(pcm[b], 8), told.transcribe_ref(pcm[b], 8)
        w = checkpoint["orc"].transcribe_ref(pcm[b:b + 1], [pcm.shape[1]], 8, tab, beg, eot, np.array([SOT, TOK0 + int(ids[b]), TRANSCRIBE], np.int32))
        for g in (ga, gt):
            assert np.array_equal(g[0], w[0][0]) and np.array_equal(bits(g[1]), bits(w[1][0])) and (g[2], g[3]) == (int(w[2][0]), int(w[3][0])), b
        assert auto.last_languages()[0].tolist() == [ids[b]]
        ta, tt = auto.process_audio(pcm[b], True)[0], told.process_audio(pcm[b], True)[0]
        assert ta == tt, b
        texts.add(ta)
        for a in (auto, told):                                               # whisper.cpp's temperature fallback armed: every attempt detects again
            a.set_decode_policy(True, seed=5)
        pa, pt = auto.process_audio(pcm[b], True)[0], told.process_audio(pcm[b], True)[0]
        assert pa == pt and auto.last_decode() == told.last_decode(), b
        assert auto.last_languages()[0].tolist() == [ids[b]]
        for a in (auto, told):
            a.set_decode_policy(False)
    auto.close()
    told.close()


def test_an_english_only_vocabulary_detects_nothing(gpu):
    hp = (80, 50, 64, 2, 2, 32, 64, 2, 2, 51864)
    en = gpu.Asr(hp=gpu.WhisperHP(*hp), seed=11)
    pcm = utterances()[:1]
    t0, _, _, l0 = en.transcribe_tokens(pcm, STEPS)
    assert en.set_language("auto") == 0 and en.prompt_tokens() == [50257, 50362]
    t1, _, _, l1 = en.transcribe_tokens(pcm, STEPS)
    wt, _, _, wl = O.OracleWhisper(O.WhisperHP(*hp), seed=11).transcribe(pcm, STEPS)
    assert np.array_equal(t1, t0) and np.array_equal(bits(l1), bits(l0)) and np.array_equal(t1, wt) and np.array_equal(bits(l1), bits(wl))
    lid, lpr = en.last_languages()
    assert lid.tolist() == [0] and lpr.tolist() == [1.0]
    with pytest.raises(gpu.TkError) as e:
        en.detect_language(pcm)
    assert e.value.code == 1001
    en.close()
