"""CPU: the string side of the text path -- prompt-attention syntax, 75-token chunking with comma backtracking / BREAK / textual-inversion
placeholders, AND-composition lists -- against the REFERENCE's parse_prompt_attention, ClassicTextProcessingEngine.tokenize_line (run with the
real CLIP tokenizer; every tokenizer call recorded and replayed here) and get_multicond_prompt_list (tests/golden/tokenize_clip_l.pt)."""
import torch

from forge_amd.backend.text_processing.classic_engine import ClassicTextProcessingEngine
from forge_amd.backend.text_processing.parsing import parse_prompt_attention
from forge_amd.modules import prompt_parser as pp
from oracle.make_golden import FakeEmbeddingDb, ReplayTokenizer

from conftest import load_golden


def test_parse_prompt_attention_vs_reference():
    g = load_golden("tokenize_clip_l.pt")
    for prompt, want in zip(g["prompts"], g["parsed"]):
        assert parse_prompt_attention(prompt, "Original") == want, prompt
    assert parse_prompt_attention("(a:1.2) [b]", "None") == [["(a:1.2) [b]", 1.0]]


def test_tokenize_line_chunking_vs_reference():
    g = load_golden("tokenize_clip_l.pt")
    eng = ClassicTextProcessingEngine(None, tokenizer=ReplayTokenizer(g["tokenizer"]), embeddings=FakeEmbeddingDb(g["emb_ids"]))
    for prompt, want in zip(g["prompts"], g["lines"]):
        chunks, count = eng.tokenize_line(prompt)
        assert count == want["count"] and len(chunks) == len(want["chunks"]), prompt
        for c, w in zip(chunks, want["chunks"]):
            assert c.tokens == w["tokens"] and c.multipliers == w["multipliers"] and [f.offset for f in c.fixes] == w["fixes"], prompt
            assert len(c.tokens) == 77
    batch_chunks, token_count = eng.process_texts(g["prompts"][:4])
    assert token_count == g["process_texts"]["token_count"] and [len(c) for c in batch_chunks] == g["process_texts"]["n_chunks"]
    assert eng.get_target_prompt_token_count(76) == 150 and eng.empty_chunk().tokens[:2] == [g["tokenizer"]["bos"], g["tokenizer"]["eos"]]


def test_multicond_prompt_list_and_objects():
    g = load_golden("tokenize_clip_l.pt")["multicond"]
    idx, flat, pidx = pp.get_multicond_prompt_list(g["prompts"])
    assert idx == g["indexes"] and list(flat) == g["flat"] and pidx == g["prompt_indexes"]

    class Model:  # encodes a text as a [2, 4] tensor filled with its length
        def get_learned_conditioning(self, texts):
            return torch.stack([torch.full((2, 4), float(len(t))) for t in texts])
    mc = pp.get_multicond_learned_conditioning(Model(), g["prompts"], steps=20)
    assert mc.shape == (len(g["prompts"]),) and [[part.weight for part in parts] for parts in mc.batch] == [[w for _, w in i] for i in idx]
    conds_list, stacked = pp.reconstruct_multicond_batch(mc, 3)
    assert conds_list[0] == [(0, 1.0), (1, 1.5), (2, 0.25)] and stacked.shape[0] == sum(len(i) for i in idx)
    # prompt editing: explicit schedules, resolved per step
    sched = pp.get_learned_conditioning(Model(), ["ab", "c"], 10, schedules=[[[4, "a"], [10, "abc"]], [[10, "c"]]])
    assert [e.end_at_step for e in sched[0]] == [4, 10]
    assert float(pp.reconstruct_cond_batch(sched, 4)[0, 0, 0]) == 1.0 and float(pp.reconstruct_cond_batch(sched, 5)[0, 0, 0]) == 3.0


def test_prompt_editing_schedules_match_the_reference_doctests():
    """Known answers: the doctest block of get_learned_conditioning_prompt_schedules (modules/prompt_parser.py:32-71; lark is not installed here,
    so the reference parser itself cannot run) and the worked example in the comment at its top (:7-13).  One doctest is left out: the reference
    marks `[{b|d{:.5]` as "not handling this right now" and its stated answer contradicts the grammar ('|' is not a plain character)."""
    g = lambda p, base=10, hires=None: pp.get_learned_conditioning_prompt_schedules([p], base, hires)[0]
    assert g("test") == [[10, "test"]]
    assert g("a [b:3]") == [[3, "a "], [10, "a b"]]
    assert g("a [b: 3]") == [[3, "a "], [10, "a b"]]
    assert g("a [[[b]]:2]") == [[2, "a "], [10, "a [[b]]"]]
    assert g("[(a:2):3]") == [[3, ""], [10, "(a:2)"]]
    assert g("a [b : c : 1] d") == [[1, "a b  d"], [10, "a  c  d"]]
    assert g("a[b:[c:d:2]:1]e") == [[1, "abe"], [2, "ace"], [10, "ade"]]
    assert g("a [unbalanced") == [[10, "a [unbalanced"]]
    assert g("a [b:.5] c") == [[5, "a  c"], [10, "a b c"]]
    assert g("((a][:b:c [d:3]") == [[3, "((a][:b:c "], [10, "((a][:b:c d"]]
    assert g("[a|(b:1.1)]") == [[i, "a" if i % 2 else "(b:1.1)"] for i in range(1, 11)]
    assert g("[fe|]male") == [[i, "female" if i % 2 else "male"] for i in range(1, 11)]
    assert g("[fe|||]male") == [[i, "female" if i % 4 == 1 else "male"] for i in range(1, 11)]
    assert g("a [b:.5] c", 10, 10) == [[10, "a b c"]]
    assert g("a [b:1.5] c", 10, 10) == [[5, "a  c"], [10, "a b c"]]
    big = "fantasy landscape with a [mountain:lake:0.25] and [an oak:a christmas tree:0.75][ in foreground::0.6][: in background:0.25] [shoddy:masterful:0.5]"
    assert g(big, 100) == [[25, "fantasy landscape with a mountain and an oak in foreground shoddy"],
                           [50, "fantasy landscape with a lake and an oak in foreground in background shoddy"],
                           [60, "fantasy landscape with a lake and an oak in foreground in background masterful"],
                           [75, "fantasy landscape with a lake and an oak in background masterful"],
                           [100, "fantasy landscape with a lake and a christmas tree in background masterful"]]
    assert g("a | b [c:3]") == [[10, "a | b [c:3]"]]   # a top-level '|' has no parse: used as is
    assert g("\\\\[not:3\\\\] (x:1.2)") == [[10, "\\\\[not:3\\\\] (x:1.2)"]]


def random_prompts(n=4000, seed=0):
    """n random strings over the syntax's alphabet (the inputs of ref_prompt_attention_random.json.gz, oracle/make_ref_fixtures.py)."""
    import random
    rnd = random.Random(seed)
    alphabet = ["a", "cat ", "(", ")", "[", "]", ":", "1.2", " ", "\\(", "\\)", "\\\\", "\\", " BREAK ", "BREAK", ",", ":0.5)", ": 1.3 )", "dog", "(((", "]]",
                ":-1)", ":.5)", "\n", "x:y"]
    return ["".join(rnd.choice(alphabet) for _ in range(rnd.randint(1, 12))) for _ in range(n)]


def test_parse_prompt_attention_randomised_against_the_reference_module():
    """4 000 random strings over the syntax's alphabet through the native parser, against what the reference's parsing.py returned for each of
    them in both modes (tests/golden/ref_prompt_attention_random.json.gz, recorded by oracle/make_ref_fixtures.py)."""
    import gzip
    import json
    import os
    from conftest import GOLDEN
    with gzip.open(os.path.join(GOLDEN, "ref_prompt_attention_random.json.gz"), "rt") as f:
        rows = json.load(f)
    prompts = random_prompts()
    assert [s for s, mode, _ in rows] == [s for s in prompts for _ in ("Original", "None")]
    for s, mode, want in rows:
        assert parse_prompt_attention(s, mode) == want, repr(s)


def test_prompt_schedule_invariants():
    """Properties of the prompt-editing schedules that hold for any input: ends at the last step, strictly increasing marks, text without
    constructs is returned unchanged, and rendering is idempotent on construct-free output."""
    import random
    rnd = random.Random(1)
    alphabet = ["a", " b", "[", "]", ":", "|", "(", ")", "3", ".5", " ", "cat", "\\[", "1.5", "0"]
    for _ in range(3000):
        s = "".join(rnd.choice(alphabet) for _ in range(rnd.randint(0, 14)))
        for steps, hires in ((10, None), (7, 12)):
            sched = pp.get_learned_conditioning_prompt_schedules([s], steps, hires)[0]
            total = hires if hires is not None else steps
            marks = [m for m, _ in sched]
            assert marks[-1] == total and marks == sorted(set(marks)) and all(1 <= m <= total for m in marks), (s, sched)
            if not any(ch in s for ch in "[|"):
                assert sched == [[total, s]], (s, sched)


def test_t5_engine_tokenize_line_vs_reference():
    """T5TextProcessingEngine.tokenize_line (backend/text_processing/t5_engine.py:68-112) run by the reference with the real T5 tokenizer, replayed:
    EOS = 1 appended, padding 0 to 256, BREAK opens a chunk, emphasis weights per token, the bracket-token multiplier table."""
    from forge_amd.backend.text_processing.t5_engine import T5TextProcessingEngine
    from oracle.make_golden import ReplayT5Tokenizer
    from types import SimpleNamespace
    g = load_golden("tokenize_t5.pt")
    eng = T5TextProcessingEngine(SimpleNamespace(transformer=None), ReplayT5Tokenizer(g["tokenizer"]))
    assert eng.token_mults == g["token_mults"] and eng.comma_token == g["comma_token"]
    for prompt, want in zip(g["prompts"], g["lines"]):
        chunks, count = eng.tokenize_line(prompt)
        assert count == want["count"] and len(chunks) == len(want["chunks"]), prompt
        for c, w in zip(chunks, want["chunks"]):
            assert c.tokens == w["tokens"] and c.multipliers == w["multipliers"], prompt
            assert len(c.tokens) >= 256 and c.tokens[-1] in (0, 1)

    # __call__: one encoding per chunk, emphasis applied ("Original": multiply, restore the mean), lines cached
    calls = []

    def fake_encoder(input_ids):
        calls.append(input_ids.shape)
        return torch.ones(input_ids.shape[0], input_ids.shape[1], 4) * torch.arange(1, input_ids.shape[1] + 1).view(1, -1, 1).float()
    eng = T5TextProcessingEngine(SimpleNamespace(transformer=fake_encoder), ReplayT5Tokenizer(g["tokenizer"]))
    z = eng([g["prompts"][0], g["prompts"][1], g["prompts"][0]])
    assert z.shape == (4, 256, 4) and len(calls) == 3          # 1 + 2 chunks + the cached repeat
    assert torch.equal(z[0], z[3])
    base = torch.arange(1, 257).view(-1, 1).float().expand(256, 4)
    assert torch.allclose(z[0], base)                           # no emphasis in prompt 0: untouched
    m = torch.tensor(g["lines"][1]["chunks"][0]["multipliers"]).view(-1, 1)
    want = base * m
    assert torch.allclose(z[1], want * (base.mean() / want.mean()), rtol=1e-5)
