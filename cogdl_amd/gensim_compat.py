"""The part of gensim the reference's embedding models use, on the library's skip-gram operator:
`Word2Vec(sentences, vector_size=, window=, min_count=0, sg=1, workers=, epochs=)` and `model.wv[token]`
(cogdl/models/emb/deepwalk.py:60-70, node2vec.py:83-93, metapath2vec.py, dgk.py).  `install(skipgram=True)` registers this
module as `gensim` where the real package cannot be imported; `from gensim.models import Word2Vec, KeyedVectors` and the
submodules `gensim.models.word2vec` / `gensim.models.keyedvectors` resolve.

Served: skip-gram with negative sampling (sg=1, hs=0, negative >= 1).  CBOW (sg=0), hierarchical softmax (hs=1) and
negative=0 raise NotImplementedError.  `Doc2Vec(documents, vector_size=, window=, min_count=, dm=, sample=, workers=, epochs=,
alpha=)` with `TaggedDocument(words, tags)` (cogdl/models/emb/graph2vec.py:99-110, `gensim.models.doc2vec`) is served as
PV-DBOW on the library's doc2vec_dbow operator, exactly where gensim selects it: gensim computes sg = (1 + dm) % 2 and trains
DBOW when that is truthy, which covers dm=0 and the 1e-4 the reference's CLI path passes; a dm that selects PV-DM, hs=1,
negative < 1 and dbow_words raise NotImplementedError.  `model[tag]`, `model.dv[tag]` and `model.docvecs[tag]` return the
document's row, `model.wv` holds the (untrained, as in gensim's pure DBOW) word vectors.  Tokens are any hashables; the vocabulary is in first-seen
order (gensim sorts by frequency: only `model.wv[token]` is order-free).  Ragged sentences are padded with -1; sentences
longer than 1024 tokens are cut into pieces of 1024 (gensim cuts at 10,000).  Training runs on the GPU when one is visible
(`device=` overrides), on the host twin otherwise.  `workers=1` is the serial, reproducible and slow mode, as in gensim;
every other value trains rows concurrently.  The draws are Philox's, not gensim's generator.
"""
import collections
import sys
import types

import numpy as np
import torch

from . import _rebind
from .operators import pvdbow as _pvdbow
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


class Vocab(object):
    """gensim 3's per-word record, which cogdl/models/emb/gatne.py:4,363 still builds: attributes from keywords (`count`,
    `index`), ordered by count."""

    def __init__(self, **kwargs):
        self.count = 0
        self.__dict__.update(kwargs)

    def __lt__(self, other):
        return self.count < other.count

    def __str__(self):
        return "%s<%s>" % (self.__class__.__name__, ", ".join("%s:%r" % kv for kv in sorted(self.__dict__.items())))


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


TaggedDocument = collections.namedtuple("TaggedDocument", "words tags")


class Doc2Vec(object):
    def __init__(self, documents=None, vector_size=100, window=5, min_count=5, dm=1, sample=1e-3, workers=3, epochs=10, alpha=0.025,
                 min_alpha=1e-4, negative=5, seed=None, device=None, hs=0, dbow_words=0, ns_exponent=0.75):
        if not (1 + dm) % 2:  # gensim's own selection: sg = (1 + dm) % 2, DBOW when truthy
            raise NotImplementedError("Doc2Vec: only PV-DBOW is served, not PV-DM (dm=%r)" % (dm,))
        if int(hs) != 0:
            raise NotImplementedError("Doc2Vec: hierarchical softmax (hs=1) is not served")
        if int(negative) < 1:
            raise NotImplementedError("Doc2Vec: negative sampling is the only objective served (negative >= 1)")
        if dbow_words:
            raise NotImplementedError("Doc2Vec: dbow_words is not served")
        self.vector_size, self.window, self.min_count, self.epochs = int(vector_size), int(window), int(min_count), int(epochs)
        self.alpha, self.min_alpha, self.sample, self.negative = float(alpha), float(min_alpha), float(sample), int(negative)
        self.ns_exponent, self.workers, self.seed, self.device, self.dm = float(ns_exponent), int(workers), seed, device, dm
        self.wv, self.dv = KeyedVectors(self.vector_size), KeyedVectors(self.vector_size)
        self.syn1neg = np.zeros((0, self.vector_size), dtype=np.float32)
        if documents is not None:
            self._train(documents)

    @property
    def docvecs(self):
        return self.dv

    def __getitem__(self, tag):
        return self.dv[tag]

    def _train(self, documents):
        per_tag = {}  # tag -> the words of every document that carries it, in first-seen order of the tags
        for doc in documents:
            for tag in doc.tags:
                per_tag.setdefault(tag, []).extend(doc.words)
        count = {}
        for words in per_tag.values():
            for tok in words:
                count[tok] = count.get(tok, 0) + 1
        index = {}
        for words in per_tag.values():
            for tok in words:
                if tok not in index and count[tok] >= self.min_count:
                    index[tok] = len(index)
        self.wv.key_to_index, self.wv.index_to_key = index, list(index)
        self.dv.index_to_key = list(per_tag)
        self.dv.key_to_index = {tag: k for k, tag in enumerate(self.dv.index_to_key)}
        rows = [[index[tok] for tok in words if tok in index] for words in per_tag.values()]
        g, v = len(rows), len(index)
        device = self.device if self.device is not None else ("cuda" if torch.cuda.is_available() else "cpu")
        seed = _pvdbow._seed(self.seed)
        doc_ptr = torch.tensor(np.concatenate([[0], np.cumsum([len(r) for r in rows], dtype=np.int64)]), dtype=torch.long)
        words = torch.tensor([t for r in rows for t in r], dtype=torch.long)
        if v == 0:  # no word is kept: nothing to train on
            dv, syn1 = _pvdbow.init_tables(g, 1, self.vector_size, seed, "cpu")
        else:
            dv, syn1 = _pvdbow.doc2vec_dbow(doc_ptr.to(device), words.to(device), v, dim=self.vector_size, negative=self.negative,
                                            epochs=self.epochs, alpha=self.alpha, min_alpha=self.min_alpha, sample=self.sample,
                                            ns_exponent=self.ns_exponent, seed=seed, workers=self.workers)
        self.dv.vectors, self.syn1neg = dv.cpu().numpy(), syn1.cpu().numpy()[:v]
        self.wv.vectors = _sgns.init_tables(v, self.vector_size, seed, "cpu")[0].numpy() if v else np.zeros((0, self.vector_size), np.float32)


def _submodule(name, **names):
    mod = types.ModuleType(__name__ + "." + name)
    mod.__dict__.update(names)
    return mod


# the module layout of gensim that the reference imports from
models = _submodule("models", Word2Vec=Word2Vec, KeyedVectors=KeyedVectors, Doc2Vec=Doc2Vec)
models.word2vec = _submodule("models.word2vec", Word2Vec=Word2Vec)
models.keyedvectors = _submodule("models.keyedvectors", KeyedVectors=KeyedVectors, Vocab=Vocab)
models.doc2vec = _submodule("models.doc2vec", Doc2Vec=Doc2Vec, TaggedDocument=TaggedDocument)
__path__ = []  # (a package as far as `import gensim.models` is concerned; the submodules are registered by install())

SUBMODULES = {"gensim.models": models, "gensim.models.word2vec": models.word2vec, "gensim.models.keyedvectors": models.keyedvectors,
              "gensim.models.doc2vec": models.doc2vec}


def register():
    """Serve this module as `gensim` (install(skipgram=True) calls it only when the real package is absent)."""
    for name, mod in [("gensim", sys.modules[__name__])] + list(SUBMODULES.items()):
        _rebind.put("gensim", sys.modules, name, mod)


def unregister():
    _rebind.undo("gensim")
