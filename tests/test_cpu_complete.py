"""Host side of BigramLanguageModel.complete / score, without a GPU: the command line of
replicatinggpt_amd.sample, prompt packing, stop-set words, argument validation, and the C-ABI entry
cg_decode_emit (header symbol, ctypes signature, torch op)."""
import ctypes

import pytest
import torch


# ---------------------------------------------------------------------------------------
# the command line
# ---------------------------------------------------------------------------------------
def test_sample_cli_one_prompt_is_the_generate_call():
    from replicatinggpt_amd import sample
    a = sample.parse_args(["--model", "m.pth"])
    assert (a.prompt, a.prompts, a.ragged, a.stop, a.logprobs, a.prompt_file) == ("", [""], False, "", False, None)
    a = sample.parse_args(["--model", "m.pth", "--prompt", "ROMEO:", "--num-samples", "3"])
    assert (a.prompt, a.prompts, a.ragged) == ("ROMEO:", ["ROMEO:"], False)


def test_sample_cli_several_prompts_stop_and_logprobs(tmp_path):
    from replicatinggpt_amd import sample
    a = sample.parse_args(["--model", "m.pth", "--prompt", "ROMEO:", "--prompt", "First Citizen:", "--prompt", ""])
    assert a.prompts == ["ROMEO:", "First Citizen:", ""] and a.ragged
    f = tmp_path / "prompts.txt"
    f.write_text("JULIET:\n\nO Romeo, Romeo!\n", encoding="utf-8")
    a = sample.parse_args(["--model", "m.pth", "--prompt", "ROMEO:", "--prompt-file", str(f)])
    assert a.prompts == ["ROMEO:", "JULIET:", "", "O Romeo, Romeo!"] and a.ragged
    a = sample.parse_args(["--model", "m.pth", "--prompt-file", str(f)])
    assert a.prompts == ["JULIET:", "", "O Romeo, Romeo!"] and a.ragged
    for extra in (["--stop", "\n."], ["--logprobs"]):
        a = sample.parse_args(["--model", "m.pth", "--prompt", "ROMEO:"] + extra)
        assert a.ragged and a.prompts == ["ROMEO:"] and a.prompt == "ROMEO:"
    assert a.logprobs and sample.parse_args(["--model", "m.pth", "--stop", "\n."]).stop == "\n."


def test_sample_cli_encoding_of_prompts_and_stop():
    from replicatinggpt_amd import sample
    from replicatinggpt_amd.data import DEFAULT_INPUT
    tok = sample.load_tokenizer(DEFAULT_INPUT)
    rows = sample.encode_prompts(tok, ["ROMEO:", "", "Oh"], 2)
    assert [r.tolist() for r in rows] == [tok.encode("ROMEO:")] * 2 + [[0]] * 2 + [tok.encode("Oh")] * 2
    assert all(r.dtype == torch.long and r.dim() == 1 for r in rows)
    assert sample.encode_stop(tok, "") == []
    assert sample.encode_stop(tok, ".\n.") == sorted({tok.stoi["."], tok.stoi["\n"]})
    with pytest.raises(ValueError, match="vocabulary") as e:
        sample.encode_stop(tok, ".~#")
    assert "~" in str(e.value) and "#" in str(e.value) and "--stop" in str(e.value)
    with pytest.raises(ValueError, match="vocabulary") as e:
        sample.encode_prompts(tok, ["ROMEO:", "JULIET~"], 1)
    assert "~" in str(e.value) and "--prompt" in str(e.value)


def test_sample_cli_logprob_line():
    from replicatinggpt_amd import sample
    lp = torch.tensor([0.0, -1.0, -2.0, -3.0, -0.5, 0.0])
    assert sample.logprob_line(lp, 3, 5) == "[2 new tokens: mean log-prob -1.7500, 2.5247 bits per character]"
    assert sample.logprob_line(lp, 3, 3).startswith("[2 prompt tokens: mean log-prob -1.5000")
    assert sample.logprob_line(lp, 1, 1) == "[no token to score]"


# ---------------------------------------------------------------------------------------
# packing and validation
# ---------------------------------------------------------------------------------------
def test_pack_prompts_list_and_pair():
    from replicatinggpt_amd.completion import pack_prompts
    rows = [torch.tensor([5, 6, 7]), torch.tensor([9]), torch.tensor([1, 2, 3, 4, 5])]
    idx, lens = pack_prompts(rows)
    assert lens.tolist() == [3, 1, 5] and lens.dtype == torch.int64
    assert idx.tolist() == [[5, 6, 7, 0, 0], [9, 0, 0, 0, 0], [1, 2, 3, 4, 5]] and idx.dtype == torch.int64
    wide = torch.full((3, 8), 11, dtype=torch.int64)
    wide[:, :5] = idx
    idx2, lens2 = pack_prompts((wide, torch.tensor([3, 1, 5])))
    assert lens2.tolist() == [3, 1, 5] and idx2.shape == (3, 5) and torch.equal(idx2, wide[:, :5])
    idx3, lens3 = pack_prompts((wide, [8, 8, 2]))
    assert idx3.shape == (3, 8) and lens3.tolist() == [8, 8, 2]
    for bad, msg in (([], "no prompt"), ([torch.tensor([1]), torch.zeros(0, dtype=torch.int64)], r"prompts\[1\] is empty"),
                     ([torch.tensor([1.0])], "int64"), ([torch.zeros((1, 2), dtype=torch.int64)], "1-D"),
                     ((wide, torch.tensor([3, 0, 5])), "length"), ((wide, torch.tensor([3, 9, 5])), "length"),
                     ((wide, torch.tensor([3, 5])), "lengths"), ((wide.float(), torch.tensor([3, 1, 5])), "int64")):
        with pytest.raises(ValueError, match=msg):
            pack_prompts(bad)


def test_stop_words_bits():
    from replicatinggpt_amd.completion import stop_words
    assert stop_words((), 65) is None and stop_words([], 1024) is None
    w = stop_words([0, 46, 64], 65)
    assert w.dtype == torch.int64 and w.tolist() == [1 | (1 << 46), 1]
    w = stop_words(range(65), 65)
    assert w.tolist() == [-1, 1]                                   # 64 bits set: -1 as int64
    w = stop_words([63, 127, 1023], 1024)
    assert w.numel() == 16 and w[0].item() == -(1 << 63) and w[1].item() == -(1 << 63) and w[15].item() == -(1 << 63)
    assert ctypes.c_uint64(w[0].item()).value == 1 << 63
    for bad in ([65], [-1], [3, 1024]):
        with pytest.raises(ValueError, match="stop_tokens"):
            stop_words(bad, 65)


def _cpu_model():
    from replicatinggpt_amd import BigramLanguageModel, GPTConfig
    return BigramLanguageModel(GPTConfig(block_size=8, n_embd=16, n_head=2, n_layers=1, dropout=0.0)).eval()


def test_complete_validates_before_it_looks_at_the_device():
    m = _cpu_model()
    ok = [torch.tensor([1, 2, 3]), torch.tensor([4])]
    for args, kw, msg in (
            (([torch.tensor([1]), torch.zeros(0, dtype=torch.int64)], 4), {}, "empty"),
            (([], 4), {}, "no prompt"),
            ((ok, -1), {}, "max_new_tokens"),
            ((ok, 1.5), {}, "max_new_tokens"),
            ((ok, 4), {"stop_tokens": [65]}, "stop_tokens"),
            ((ok, 4), {"stop_tokens": [3, -2]}, "stop_tokens"),
            ((ok, 4), {"pad_token": 65}, "pad_token"),
            ((ok, 4), {"pad_token": -1}, "pad_token"),
            ((ok, 4), {"poll_every": -1}, "poll_every"),
            (([torch.tensor([1, 65])], 4), {}, "outside the vocabulary"),
            ((ok, 4), {"temperature": 0.0}, "temperature"),
            ((ok, 4), {"greedy": True, "top_k": 5}, "greedy"),
    ):
        with pytest.raises(ValueError, match=msg):
            m.complete(*args, **kw)


def test_complete_and_score_need_a_gpu():
    """Valid arguments on a CPU model: a clear error, not a fallback."""
    m = _cpu_model()
    with pytest.raises(RuntimeError, match="GPU"):
        m.complete([torch.tensor([1, 2, 3])], 4, stop_tokens=[0])
    with pytest.raises(RuntimeError, match="GPU"):
        m.score([torch.tensor([1, 2, 3])])


# ---------------------------------------------------------------------------------------
# the C ABI
# ---------------------------------------------------------------------------------------
def test_decode_emit_symbol_signature_and_op():
    from replicatinggpt_amd import _lib, ops  # noqa: F401
    assert "cg_decode_emit" in _lib.header_symbols()
    res, args = _lib._SIGS["cg_decode_emit"]
    P, i64 = ctypes.c_void_p, ctypes.c_int64
    # logits, ldl, V, B, mode, params, seed, len, prompt_len, limit, end, stop_bits, pad, idx, ld, logprob, stream
    assert res is ctypes.c_int
    assert args == [P, i64, i64, i64, ctypes.c_int, P, P, P, P, P, P, P, P, P, i64, P, P]
    lib = _lib.load()
    assert hasattr(lib, "cg_decode_emit") and lib.cg_decode_emit.argtypes == args
    # argument checks come before any launch: null pointers and bad sizes are CG_EINVAL with a message
    assert lib.cg_decode_emit(None, 65, 65, 1, 0, None, None, None, None, None, None, None, None, None, 4, None, None) != 0
    assert b"null pointer" in lib.cg_last_error_string()
    for V, ldl, mode, word in ((0, 65, 0, b"V = 0"), (1025, 1025, 0, b"V = 1025"), (65, 64, 0, b"ldl = 64"),
                               (65, 65, 3, b"mode = 3")):
        assert lib.cg_decode_emit(None, ldl, V, 1, mode, None, None, None, None, None, None, None, None, None, 4, None,
                                  None) != 0
        assert word in lib.cg_last_error_string(), (word, lib.cg_last_error_string())
    assert hasattr(torch.ops.charpt, "decode_emit")
    schema = str(torch.ops.charpt.decode_emit.default._schema)
    assert "Tensor(a" in schema and "logprob" in schema and "stop_bits" in schema
    # the old samplers keep their entries
    assert hasattr(lib, "cg_decode_sample") and hasattr(lib, "cg_decode_sample_filtered")
