"""CPU-side checks of prompt-lookup speculation under seeded sampling: the library and ops.spec_counters check
their arguments before any launch, generate() admits do_sample=True with a seed and with a seed only, and
completion() / the command lines pass the seed on."""
import pytest
import torch


def test_bad_arguments_are_refused_by_the_library():
    from valley_amd import lib_spec_sample
    h = lib_spec_sample.load()
    ok = 4096
    for args in ((None, 3, 64, ok), (ok, 3, 64, None), (ok, 0, 64, ok), (ok, 8, 64, ok), (ok, 3, 3, ok), (ok, 3, 0, ok),
                 (ok + 2, 3, 64, ok), (ok, 3, 64, ok + 1)):
        assert h.vly_spec_counters(*args, None) == -22, args
        assert b"vly_spec_counters" in h.vly_spec_sample_last_error()


def test_spec_counters_checks_its_arguments_before_any_launch():
    from valley_amd import lib, ops
    i32 = lambda *s: torch.zeros(s, dtype=torch.int32)           # noqa: E731
    for k in (0, 8, -1):
        with pytest.raises(ValueError, match=r"k must be in \[1, 7\]"):
            ops.spec_counters(i32(1), k, 64, i32(max(k, 0) + 1))
    with pytest.raises(ValueError, match="out must be int32"):   # shorter than k + 1
        ops.spec_counters(i32(1), 3, 64, i32(3))
    with pytest.raises(ValueError, match="out must be int32"):
        ops.spec_counters(i32(1), 3, 64, torch.zeros((4,), dtype=torch.int64))
    with pytest.raises(ValueError, match="out must be int32"):
        ops.spec_counters(i32(1), 3, 64, torch.zeros((4,), dtype=torch.float32))
    with pytest.raises(ValueError, match="pos must be an int32 tensor of 1 element"):
        ops.spec_counters(i32(2), 3, 64, i32(4))
    with pytest.raises(ValueError, match="pos must be an int32 tensor of 1 element"):
        ops.spec_counters(torch.zeros((1,), dtype=torch.int64), 3, 64, i32(4))
    with pytest.raises(ValueError, match="pos must be an int32 tensor of 1 element"):
        ops.spec_counters(5, 3, 64, i32(4))
    with pytest.raises(ValueError, match="ctx_max"):
        ops.spec_counters(i32(1), 3, 3, i32(4))
    with pytest.raises(lib.ValleyHipError):                      # all fine: no CPU compute path
        ops.spec_counters(i32(1), 3, 64, i32(4))
    with pytest.raises(lib.ValleyHipError):
        ops.spec_counters(i32(1), 7, 8, i32(8))


def stub_model():
    from valley_amd import valley_model as vm

    class Stub(vm.ValleyLlamaForCausalLM):
        def __init__(self):                                      # the checks come before the model is touched
            pass

    return Stub()


def test_seeded_sampling_passes_the_refusal_and_unseeded_does_not(monkeypatch):
    m = stub_model()
    ids = torch.zeros((1, 4), dtype=torch.long)
    reached = []

    def fake_spec(*a, **kw):
        reached.append((a, kw))
        raise RuntimeError("first launch")

    from valley_amd import generation
    monkeypatch.setattr(generation, "_generate_spec", fake_spec)
    for seed in (1, [1], (7,), 0, (1 << 64) - 1):
        with pytest.raises(RuntimeError, match="first launch"):  # (fails where the call is still refused: ValueError, do_sample)
            m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=seed)
    assert len(reached) == 5
    # the spec tuple carries the one row's seed, the sampling parameters follow it
    kw = reached[1][1]
    assert kw["spec"] == (3, 2, 1) and kw["do_sample"] is True
    with pytest.raises(RuntimeError, match="first launch"):      # a seed does not get in the way of a greedy call
        m.generate(ids, prompt_lookup_num_tokens=3, seed=4)
    del reached[:]
    with pytest.raises(ValueError, match="do_sample") as e:
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True)
    assert "seed=" in str(e.value)
    with pytest.raises(ValueError, match="do_sample"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, temperature=0.2, top_k=50)
    for bad in ([1, 2], [], (3, 4, 5)):
        with pytest.raises(ValueError, match="one seed"):
            m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=bad)
    for bad in (-1, 1 << 64, 1.5, True, "7", [2.0]):
        with pytest.raises(ValueError, match="seed must be"):
            m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=bad)
    # every other refusal stands with a seed
    with pytest.raises(ValueError, match="num_beams"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, num_beams=2)
    with pytest.raises(ValueError, match="logits processors"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, repetition_penalty=1.2)
    with pytest.raises(ValueError, match="output_logprobs"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, output_logprobs=True, return_dict_in_generate=True)
    with pytest.raises(ValueError, match="one prompt row"):
        m.generate(torch.zeros((2, 4), dtype=torch.long), prompt_lookup_num_tokens=3, do_sample=True, seed=[1, 2])
    with pytest.raises(ValueError, match="use_graph"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, use_graph=None)
    assert not reached


def test_seeded_call_on_a_real_stub_is_not_refused():
    """Without the monkeypatched body: whatever a model without weights raises, it is not the do_sample refusal."""
    m = stub_model()
    ids = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(Exception) as e:
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1)
    assert not (isinstance(e.value, ValueError) and "do_sample" in str(e.value)), e.value


def test_sampling_parameters_are_checked_before_the_prefill():
    m = stub_model()
    ids = torch.zeros((1, 4), dtype=torch.long)
    with pytest.raises(ValueError, match="top_p"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, top_p=0.0)
    with pytest.raises(ValueError, match="top_k"):
        m.generate(ids, prompt_lookup_num_tokens=3, do_sample=True, seed=1, top_k=-2)


def test_completion_and_the_command_lines_pass_the_seed_through(monkeypatch, capsys):
    from tests.fake_tokenizer import FakeTokenizer
    from valley_amd import cli
    m = stub_model()
    seen = {}

    def fake_generate(input_ids=None, **kw):
        seen.clear()
        seen.update(kw)
        return torch.cat([input_ids, torch.full((1, 2), 7, dtype=input_ids.dtype)], dim=1)

    tok = FakeTokenizer(300)
    monkeypatch.setattr(type(m), "device", property(lambda self: torch.device("cpu")), raising=False)
    monkeypatch.setattr(m, "build_inputs", lambda tokenizer, message: type("I", (), {"input_ids": [[1, 5, 6, 7]]})(), raising=False)
    monkeypatch.setattr(m, "generate", fake_generate, raising=False)
    monkeypatch.setattr(m, "process_response", lambda outs: outs, raising=False)
    video = torch.zeros((3, 2, 224, 224))
    m.completion(tok, video, [], {"max_new_tokens": 4, "do_sample": True, "prompt_lookup_num_tokens": 3, "seed": 11})
    assert seen["seed"] == 11 and seen["prompt_lookup_num_tokens"] == 3 and seen["do_sample"] is True
    m.completion(tok, video, [], {"max_new_tokens": 4})
    assert "seed" not in seen and "prompt_lookup_num_tokens" not in seen

    # the options
    a = cli.parse_args(["--prompt-lookup", "3", "--sample", "--seed", "9"])
    assert (a.prompt_lookup, a.sample, a.seed) == (3, True, 9)
    a = cli.parse_args([])
    assert (a.prompt_lookup, a.sample, a.seed) == (None, False, None)
    c = cli.conv_parse_args(["--prompt-lookup", "5", "--seed", "4"])
    assert (c.prompt_lookup, c.seed) == (5, 4)
    c = cli.conv_parse_args([])
    assert (c.prompt_lookup, c.seed) == (None, None)

    calls = {}

    class M:
        def completion(self, tokenizer, video, turns, gen, device):
            calls.clear()
            calls.update(gen)
            return ["ok"]

    monkeypatch.setattr(cli, "load", lambda *a, **k: (M(), None))
    monkeypatch.setattr(cli, "_require_gpu", lambda: torch.device("cpu"))
    monkeypatch.setattr(cli, "_PROCESS_SEED", None)
    cli.main(cli.parse_args([]))
    assert calls == cli.GREEDY
    cli.main(cli.parse_args(["--prompt-lookup", "5"]))           # greedy: no seed is drawn
    assert calls == dict(cli.GREEDY, prompt_lookup_num_tokens=5) and cli._PROCESS_SEED is None
    cli.main(cli.parse_args(["--sample"]))
    assert calls == cli.SAMPLED and cli._PROCESS_SEED is None
    cli.main(cli.parse_args(["--sample", "--prompt-lookup", "3", "--seed", "9"]))
    assert calls == dict(cli.SAMPLED, prompt_lookup_num_tokens=3, seed=9) and cli._PROCESS_SEED is None
    capsys.readouterr()
    cli.main(cli.parse_args(["--sample", "--prompt-lookup", "3"]))
    drawn = calls["seed"]
    assert calls == dict(cli.SAMPLED, prompt_lookup_num_tokens=3, seed=drawn) and 0 <= drawn < 1 << 62
    assert str(drawn) in capsys.readouterr().err                 # printed, so the run can be repeated
    cli.main_v2("v.mp4", prompt_lookup=2)
    assert calls == dict(cli.SAMPLED, prompt_lookup_num_tokens=2, seed=drawn)     # once per process
    assert capsys.readouterr().err == ""
    cli.main_v2("v.mp4")
    assert calls == cli.SAMPLED

    # the conversation's generate call: today's arguments without the options, the three new ones with them
    gen_calls = []

    class G:
        def generate(self, input_ids, **kw):
            gen_calls.append(kw)
            return torch.cat([input_ids, torch.full((1, 2), 7, dtype=input_ids.dtype)], dim=1)

    from valley_amd import video as V
    monkeypatch.setattr(V, "KeywordsStoppingCriteria", lambda *a, **k: "stop")
    conv = type("C", (), {"sep": "###"})()
    ids = torch.tensor([[1, 5, 6]])
    cli.assistant_out(G(), conv, tok, ids, torch.zeros((2, 3, 224, 224)))
    assert set(gen_calls[-1]) == {"images", "do_sample", "temperature", "max_new_tokens", "stopping_criteria"}
    cli.assistant_out(G(), conv, tok, ids, torch.zeros((2, 3, 224, 224)), prompt_lookup=3)
    assert gen_calls[-1]["prompt_lookup_num_tokens"] == 3 and gen_calls[-1]["seed"] == drawn and gen_calls[-1]["do_sample"] is True
    cli.assistant_out(G(), conv, tok, ids, torch.zeros((2, 3, 224, 224)), prompt_lookup=3, seed=21)
    assert gen_calls[-1]["seed"] == 21
