"""The part of gensim the reference's embedding models use, on the library's skip-gram operator:
`Word2Vec(sentences, vector_size=, window=, min_count=0, sg=1, workers=, epochs=)` and `model.wv[token]`
(cogdl/models/emb/deepwalk.py:60-70, node2vec.py:83-93, metapath2vec.py, dgk.py).  `install(skipgram=True)` registers this
module as `gensim` where the real package cannot be imported; `from gensim.models import Word2Vec, KeyedVectors` and the
submodules `gensim.models.word2vec` / `gensim.models.keyedvectors` resolve.

Served: skip-gram with negative sampling (sg=1, hs=0, negative >= 1).  CBOW (sg=0), hierarchical softmax (hs=1) and
negative=0 raise NotImplementedError; Doc2Vec is not served.  Tokens are any hashables; the vocabulary is in first-seen
order (gensim sorts by frequency: only `model.wv[token]` is order-free).  Ragged sentences are padded with -1; sentences
longer than 1024 tokens are cut into pieces of 1024 (gensim cuts at 10,000).  Training runs on the GPU when one is visible
(`device=` overrides), on the host twin otherwise.  `workers=1` is the serial, reproducible and slow mode, as in gensim;
every other value trains rows concurrently.  The draws are Philox's, not gensim's generator.
"""
import sys
import types

import numpy as np
import torch

from . import _rebind
from .operators import sgns as _sgns


class KeyedVectors(object):
    def __init__(self, vector_size=0):
        self.vector_size = int(vector_size)
        self.index_to_key = []
        self.key_to_index = {}
        self.vectors = np.zeros((0, self.vector_size), dtype=np.float32)

    def __getitem__(self, key):
        if isinstance(key, (list, np.ndarray)):
            return np.vstack([self.vectors[self.key_to_index[k]] for k in key])
        return self.vectors[self.key_to_index[key]]

    def get_vector(self, key):
        return self[key]

    def __contains__(self, key):
        return key in self.key_to_index

    def __len__(self):
        return len(self.index_to_key)


class Word2Vec(object):
    def __init__(self, sentences=None, vector_size=100, alpha=0.025, window=5, min_count=5, sample=1e-3, seed=None, workers=3,
                 min_alpha=1e-4, sg=0, hs=0, negative=5, ns_exponent=0.75, epochs=5, device=None):
        if int(sg) != 1:
            raise NotImplementedError("Word2Vec: only skip-gram (sg=1) is served, not CBOW")
        if int(hs) != 0:
            raise NotImplementedError("Word2Vec: hierarchical softmax (hs=1) is not served")
        if int(negative) < 1:
            raise NotImplementedError("Word2Vec: negative sampling is the only objective served (negative >= 1)")
        self.vector_size, self.window, self.min_count, self.epochs = int(vector_size), int(window), int(min_count), int(epochs)
        self.alpha, self.min_alpha, self.sample, self.negative = float(alpha), float(min_alpha), float(sample), int(negative)
        self.ns_exponent, self.workers, self.seed, self.device = float(ns_exponent), int(workers), seed, device
        self.wv = KeyedVectors(self.vector_size)
        self.syn1neg = np.zeros((0, self.vector_size), dtype=np.float32)
        if sentences is not None:
            self._train(sentences)

    def _train(self, sentences):
        sentences = [list(s) for s in sentences]
        count = {}
        for s in sentences:
            for tok in s:
                count[tok] = count.get(tok, 0) + 1
        index = {}
        for s in sentences:
            for tok in s:
                if tok not in index and count[tok] >= self.min_count:
                    index[tok] = len(index)
        self.wv.key_to_index, self.wv.index_to_key = index, list(index)
        rows = []
        for s in sentences:
            ids = [index[tok] for tok in s if tok in index]
            rows.extend(ids[k:k + _sgns.MAX_LENGTH] for k in range(0, len(ids), _sgns.MAX_LENGTH))
        v = len(index)
        if v == 0 or not rows:
            self.wv.vectors = np.zeros((v, self.vector_size), dtype=np.float32)
            return
        width = max(len(r) for r in rows)
        walks = np.full((len(rows), width), -1, dtype=np.int64)
        for k, r in enumerate(rows):
            walks[k, :len(r)] = r
        device = self.device if self.device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        syn0, syn1 = _sgns.skipgram(torch.from_numpy(walks).to(device), v, dim=self.vector_size, window=self.window,
                                    negative=self.negative, epochs=self.epochs, alpha=self.alpha, min_alpha=self.min_alpha,
                                    sample=self.sample, ns_exponent=self.ns_exponent, seed=self.seed, workers=self.workers)
        self.wv.vectors, self.syn1neg = syn0.cpu().numpy(), syn1.cpu().numpy()


def _submodule(name, **names):
    mod = types.ModuleType(__name__ + "." + name)
    mod.__dict__.update(names)
    return mod


# the module layout of gensim that the reference imports from
models = _submodule("models", Word2Vec=Word2Vec, KeyedVectors=KeyedVectors)
models.word2vec = _submodule("models.word2vec", Word2Vec=Word2Vec)
models.keyedvectors = _submodule("models.keyedvectors", KeyedVectors=KeyedVectors)
__path__ = []  # (a package as far as `import gensim.models` is concerned; the submodules are registered by install())

SUBMODULES = {"gensim.models": models, "gensim.models.word2vec": models.word2vec, "gensim.models.keyedvectors": models.keyedvectors}


def register():
    """Serve this module as `gensim` (install(skipgram=True) calls it only when the real package is absent)."""
    for name, mod in [("gensim", sys.modules[__name__])] + list(SUBMODULES.items()):
        _rebind.put("gensim", sys.modules, name, mod)


def unregister():
    _rebind.undo("gensim")
