"""The newer jobs of tests/test_gpu_literal.py without a GPU, cut short: the shipped oracle stands in for the device (which the -m gpu parity tests hold
bit-identical to it), so what runs here is the checking side of those jobs — the oracle's literal mode on the layout kinds 3 / 5 / 6, the NumPy mirror with
its pair-quartic closure, MH, the accept-rate tuner and dual averaging, the layout each job expects, its acceptance window and its tolerances.  A job whose
inputs or checkers rot fails here, before any GPU time is spent on it.  CPU only (-m "not gpu")."""
import pytest

import test_gpu_literal as T

# transitions kept of each job (the full lengths run under -m gpu and in `python tests/test_gpu_literal.py`); the dual-averaging job is short already and runs
# whole, since its tolerances belong to its length
CUT = {name: 25 for name in T.NEW_JOB_NAMES}
CUT.update(pair_quartic_slice_d100=6, pair_quartic_slice_d37=6, split_hmc_dense_d512=12)


def test_job_names_are_the_jobs():
    jobs = T._jobs()
    assert tuple(jobs.keys()) == T.JOB_NAMES
    assert set(CUT) == set(T.NEW_JOB_NAMES)
    for name in T.NEW_JOB_NAMES:
        job = jobs[name]
        assert "layout" in job, name
        assert ("accept" in job) == (job["kw"]["sampler"] != T.L.SAMPLER_SLICE), name       # every MH / MALA / HMC job has its acceptance window
        assert job.get("accept", T.ACCEPT_WINDOW) == (0.2, 0.9), name
        if job["kw"].get("tuner", 0) != T.L.TUNER_DUAL_AVERAGING:
            assert not {"rtol", "mirror_rtol", "gtol"} & set(job), name                        # 1e-12 / 1e-9 for everything but dual averaging
        else:
            assert job["rtol"] <= 1e-9 and job["gtol"] <= 1e-9 and job["mirror_rtol"] <= 1e-7, name


@pytest.mark.parametrize("name", T.NEW_JOB_NAMES)
def test_new_jobs_pass_their_checks_with_the_oracle_standing_in(name):
    r = T.check_job(name, T._stand_in_run, max_steps=CUT[name])
    print(r)
    assert r["transitions"] == min(CUT[name], T._jobs()[name]["nsteps"])
    assert r["decisions_vs_literal"] == 3 * T.BLOCK * r["transitions"] and r["decisions_vs_mirror"] == T.MIRROR_CHAINS * r["transitions"]
    assert r["dev_vs_literal"] <= T._jobs()[name].get("rtol", 1e-12)
