"""-m gpu: a sibling tile that times out is not the caller's problem.

Windows above 64 informative rows run on sibling tiles of the fused f16 stack, which wait for each other's keys across
workgroups; a tile that gives up leaves a sticky error word on the context.  The fetch that finds it repeats the job's model
pass (and its consensus pass) once with those windows on the layer-by-layer kernels, and the context stays usable.  The
fault is injected through herro_debug_sib_fault (the word a timed-out tile writes); both paths are held to the same 1e-3
contract against the twin elsewhere, so here they are compared with each other."""
import numpy as np
import pytest

import gpu_common as G
from herro_amd import api, synth

pytestmark = pytest.mark.gpu


def _close(a, b):
    if len(a) != len(b):
        return abs(len(a) - len(b)) <= 2
    return sum(x != y for x, y in zip(a, b)) <= max(1, len(a) // 1000)


def test_fetch_repeats_the_pass_without_sibling_tiles():
    sb = synth.generate(2, 2 * 4096, 32, seed=synth.SEED + 71, p_snp=0.03)
    c = G.ctx()
    G.load_synth(c, sb)
    c.set_precision(4)
    ids = [f"read{t}" for t in range(sb.n_targets)]
    job = api.job_from_synth(c, sb, 4096)
    try:
        job.featurize(); job.infer(64, 1); job.consensus()
        nsup = [job.info(w).n_supported for w in range(job.n_windows)]
        assert max(nsup) > 64, "the case needs a window on sibling tiles"
        fa0 = job.fasta(ids)
        lg0 = [job.logits(w) for w in range(job.n_windows)]
        r0 = c.sib_retries()

        # the corrected-bases fetch finds the word: model + consensus repeated, same answer within the two paths' tolerance
        job.featurize(); job.infer(64, 1); job.consensus()
        c.sib_fault()
        fa1 = job.fasta(ids)
        assert c.sib_retries() == r0 + 1
        a = [ln for ln in fa0.splitlines()]
        b = [ln for ln in fa1.splitlines()]
        assert len(a) == len(b) and all(x == y for x, y in zip(a[::2], b[::2]))
        assert all(_close(x, y) for x, y in zip(a[1::2], b[1::2]))
        worst = 0.0
        for w in range(job.n_windows):
            if not nsup[w]:
                continue
            i1, b1 = job.logits(w)
            worst = max(worst, float(np.abs(i1 - lg0[w][0]).max()), float(np.abs(b1 - lg0[w][1]).max()))
        print(f"sibling tiles vs layer-by-layer after the repeat: max abs logit difference {worst:.3e}")
        assert worst <= 2e-3
        # small windows ran the same fused kernels both times: bit-identical
        for w in range(job.n_windows):
            if 0 < nsup[w] <= 64:
                assert np.array_equal(job.logits(w)[1], lg0[w][1])
                break

        # the logits fetch finds it too; the job is past its one repeat, so a second fault on it is reported, once, and the context goes on
        job2 = api.job_from_synth(c, sb, 4096)
        try:
            job2.featurize(); job2.infer(64, 1)
            c.sib_fault()
            i2, b2 = job2.logits(int(np.argmax(nsup)))
            assert c.sib_retries() == r0 + 2
            assert np.abs(b2 - job.logits(int(np.argmax(nsup)))[1]).max() == 0   # both on the layer-by-layer path now
            # past its one repeat the job launches no sibling tiles any more: a word raised meanwhile cannot be about ITS keys — it is served (and the
            # word is cleared: the context goes on)
            job2.infer(64, 1)
            c.sib_fault()
            i3, b3 = job2.logits(int(np.argmax(nsup)))
            assert np.array_equal(b3, b2) and c.sib_retries() == r0 + 2
            job2.infer(64, 1)
            job2.logits(0)
            assert c.sib_retries() == r0 + 2
        finally:
            job2.close()
    finally:
        job.close()
        c.set_precision(api.DEFAULT_PRECISION)


def test_two_inferred_jobs_in_flight_both_repeat():
    """the error word carries no job identity.  With two inferred jobs unfetched, the fetch that finds the word used to repeat ITS job's pass
    and clear the word — the other job's later fetch then saw a clean word and returned whatever its sibling tiles had left.  Now every job whose
    sibling-tile pass was unchecked when the word was found is repeated when it is fetched."""
    sb = synth.generate(2, 2 * 4096, 32, seed=synth.SEED + 71, p_snp=0.03)
    c = G.ctx()
    G.load_synth(c, sb)
    c.set_precision(4)
    a = api.job_from_synth(c, sb, 4096)
    b = api.job_from_synth(c, sb, 4096)
    ref = api.job_from_synth(c, sb, 4096)
    try:
        ref.featurize(); ref.infer(64, 1)
        nsup = [ref.info(w).n_supported for w in range(ref.n_windows)]
        big = int(np.argmax(nsup))
        assert nsup[big] > 64
        want = ref.logits(big)[1]                   # the sibling-tile path, clean
        r0 = c.sib_retries()
        a.featurize(); a.infer(64, 1)
        b.featurize(); b.infer(64, 1)
        c.sib_fault()                               # "a tile of A or B timed out": nobody can tell whose
        lb = b.logits(big)[1]                       # B fetches first: finds the word, repeats its pass without sibling tiles
        assert c.sib_retries() == r0 + 1
        la = a.logits(big)[1]                       # A's fetch finds a clean word — and must repeat all the same
        assert c.sib_retries() == r0 + 2
        assert np.array_equal(la, lb)               # both on the layer-by-layer path now
        assert float(np.abs(la - want).max()) <= 2e-3
        # a job inferred AFTER the word was handled is not a suspect of it
        ref.infer(64, 1)
        assert np.array_equal(ref.logits(big)[1], want) and c.sib_retries() == r0 + 2
    finally:
        a.close(); b.close(); ref.close()
        c.set_precision(api.DEFAULT_PRECISION)


def _consensus_done_job():
    """The case of the tests above with all three passes run, no fault yet: (context, job, ids, the synthetic batch)."""
    sb = synth.generate(2, 2 * 4096, 32, seed=synth.SEED + 71, p_snp=0.03)
    c = G.ctx()
    G.load_synth(c, sb)
    c.set_precision(4)
    job = api.job_from_synth(c, sb, 4096)
    try:
        job.featurize(); job.infer(64, 1); job.consensus()
        nsup = [job.info(w).n_supported for w in range(job.n_windows)]
        assert max(nsup) > 64, "the case needs a window on sibling tiles"
    except BaseException:
        job.close()
        c.set_precision(api.DEFAULT_PRECISION)
        raise
    return c, job, [f"read{t}" for t in range(sb.n_targets)], sb


def test_fasta_dev_is_the_fetch_that_finds_the_word():
    """herro_job_fasta_dev settles the pass in front of its kernels: the text it forms is the repeated pass's, which is what fasta() of the same job
    reads right after — with the three chop numbers 0 the two texts are the same bytes."""
    c, job, ids, _ = _consensus_done_job()
    try:
        r0 = c.sib_retries()
        c.sib_fault()
        text = job.fasta_dev(ids, chop_len=0, min_length=0, line_width=0)
        assert c.sib_retries() == r0 + 1
        assert text == job.fasta(ids)
        job.fasta_dev(ids, chop_len=0, min_length=0, line_width=0)
        assert c.sib_retries() == r0 + 1
    finally:
        job.close()
        c.set_precision(api.DEFAULT_PRECISION)


def test_consensus_fetch_is_the_fetch_that_finds_the_word():
    """herro_job_consensus_fetch queues its copies in front of the settle and copies again behind the repeat: what fasta() assembles from them is the
    text fasta_dev forms from the device's bases.  That alone would also hold for copies of the FIRST pass wherever the two kernel paths decode the same
    bases, so the text is held to a second job's as well, whose passes ran clean and without sibling tiles from the start (a job past its one repeat
    launches none): the same kernels on the same input, the same bytes."""
    c, job, ids, sb = _consensus_done_job()
    ref = api.job_from_synth(c, sb, 4096)
    try:
        ref.featurize(); ref.infer(64, 1)
        c.sib_fault()
        ref.logits(0)                                         # its one repeat: no sibling tiles from here on
        ref.featurize(); ref.infer(64, 1); ref.consensus()    # clean passes, layer by layer above 64 rows
        want = ref.fasta(ids)
        job.featurize(); job.infer(64, 1); job.consensus()    # (ref's word tainted this job's unchecked pass too: a fresh one, on sibling tiles)
        r0 = c.sib_retries()
        c.sib_fault()
        job.consensus_fetch()
        assert c.sib_retries() == r0 + 1
        got = job.fasta(ids)
        assert got == job.fasta_dev(ids, chop_len=0, min_length=0, line_width=0)
        assert got == want
        assert c.sib_retries() == r0 + 1
    finally:
        ref.close()
        job.close()
        c.set_precision(api.DEFAULT_PRECISION)
