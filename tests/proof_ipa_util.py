"""Helpers of the IPA proof tests: proof_util.Setup over ipa.ParamsIPA.new(k) instead of a KZG setup -- the same systems, witnesses and
witness callbacks, with prove / verify / accepts going through multiopen="ipa" and one of ipa.py's strategies.  No trapdoor and no
pairing: the package's own verifier accepts or rejects.

The proof's layout in 32-byte words follows the entry's hand-counted KZG layout (systems_util.py): the same points (instance commitments
are absorbed, not written), then one evaluation per instance query and proof instance ahead of the advice evaluations, the KZG
evaluation sections, and the opening of poly/ipa: q', one evaluation per point set, S, (L_j, R_j) for j < k, c, f."""
import importlib

import proof_util as pu
from lookup_util import to_mont
from proof_util import h2, prover, transcript, verifier

ipa = importlib.import_module("halo2_pse_amd.ipa")

_PARAMS, _SETUPS = {}, {}


def params(k):
    """ParamsIPA.new(k), derived once per session; every key of that k shares it (and its pinned generators)"""
    if k not in _PARAMS:
        h2.init()
        _PARAMS[k] = ipa.ParamsIPA.new(k)
    return _PARAMS[k]


class Setup(pu.Setup):
    """params, proving key and verifying key of one system at one k over the IPA commitment scheme"""

    def __init__(self, k=None, seed=0xC0FFEE, system=None):
        self.system = pu.system_entry() if system is None else system
        self.k = self.system.k if k is None else k
        self.n = 1 << self.k
        self.cs = self.system.cs
        self.b = self.cs.blinding_factors()
        self.u = self.n - self.b - 1
        self.seed = seed
        self.cols = self.columns(seed)
        self.params = params(self.k)
        self.fixed = [to_mont(c) for c in self.cols["fixed"]]
        self.pk = prover.ProvingKey.build(self.params, self.cs, self.fixed, self.system.copies, pu.VK_REPR)

    def prove(self, columns_per_instance=None, form="parts", resident=True, seed=b"\x07" * 32, instances=None):
        columns_per_instance = self.default_witnesses() if columns_per_instance is None else columns_per_instance
        instances = self.instances_of(columns_per_instance) if instances is None else instances
        return prover.create_proof(self.params, self.pk, instances, self.witness_fn(columns_per_instance, resident), transcript.Blake2bWrite(),
                                   seed, multiopen="ipa", form=form, resident=resident)

    def verify(self, proof_bytes, instances, strategy=None, vk=None):
        """what strategy.process returns (SingleStrategy by default: None, or IPAError)"""
        strategy = ipa.SingleStrategy(self.params) if strategy is None else strategy
        return verifier.verify_proof(self.params, self.pk.vk if vk is None else vk, instances, transcript.Blake2bRead(proof_bytes),
                                     multiopen="ipa", strategy=strategy)

    def accepts(self, proof_bytes, instances, vk=None):
        """False when the verifier refuses: a malformed proof, instances that do not fit, an opening that does not verify"""
        try:
            self.verify(proof_bytes, instances, vk=vk)
        except (transcript.TranscriptError, verifier.VerifyError, ipa.IPAError):
            return False
        return True

    # ---- the layout, in words
    def instance_eval_words(self):
        return self.system.n_instances * len(self.cs.instance_queries)

    def fields(self, proof_bytes):
        """word offsets of one field of each kind in a proof of the entry's own number of instances, from its layout and the opening's
        fixed tail"""
        e, words = self.system, len(proof_bytes) // 32
        assert len(proof_bytes) == 32 * words
        inst = self.instance_eval_words()
        q_prime = e.evaluation_words() + inst
        tail = 1 + 2 * self.k + 2                                  # S, the rounds, c, f
        point_sets = words - q_prime - 1 - tail
        assert 1 <= point_sets <= len(self.cs.advice_queries) + len(self.cs.fixed_queries) + 3, (words, q_prime, point_sets)
        out = {"advice commitment": 0, "h piece commitment": e.section("h")[0], "advice evaluation": e.layout["points"] + inst,
               "q' commitment": q_prime, "L_0": words - 2 - 2 * self.k, "L_last": words - 4, "c": words - 2, "f": words - 1}
        if inst:
            out["instance evaluation"] = e.layout["points"]
        return out


def setup(entry, k=None):
    """the Setup of a systems_util / systems_args_util entry, built once per session and k"""
    key = (entry.name, k)
    if key not in _SETUPS:
        _SETUPS[key] = Setup(k=k, system=entry)
    return _SETUPS[key]
