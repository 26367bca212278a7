"""Caption nouns -> caption-vocabulary ids (``ids_cap``): ``LVISParser.parse`` (maskrcnn_benchmark/data/datasets/helper/
parser.py:23-74) and ``COCOCapDetDataset.extract_obj`` (datasets/coco_cap_det.py:131-140).

The vocabulary is DATA read at run time from an LVIS-format categories JSON -- a list of ``{"id", "name", "synonyms"}``
(or an object with such a list under ``"categories"``); ids are 1-based there and 0-based in ``ids_cap``.

The lemmatiser is pluggable: a callable ``text -> list of lemma strings``.  ``default_lemmatizer()`` is spaCy's
``en_core_web_sm`` when it can be loaded -- the reference's -- and otherwise ``whitespace_tokens``: lower-case
whitespace tokens.  THE FALLBACK IS NOT THE REFERENCE'S LEMMATISATION: "dogs" does not become "dog", punctuation stays glued
to its word, and a hyphenated word stays one token.  For the reference's exact nouns, bake them offline into the caption
file (``"ids_cap"`` on a caption annotation wins over parsing, see data/datasets.py).
"""
import json


def whitespace_tokens(text):
    return text.lower().split()


def default_lemmatizer():
    try:
        import spacy
        nlp = spacy.load("en_core_web_sm")
    except (ImportError, OSError):
        return whitespace_tokens
    return lambda text: [token.lemma_ for token in nlp(text)]


class CaptionParser:
    def __init__(self, categories, lemmatize=None):
        self.lemmatize = lemmatize or default_lemmatizer()
        self.class_names = [""] * len(categories)
        self.look_up = {}  # lemmatised synonym phrase -> 0-based vocabulary id; a later phrase overwrites an earlier one
        for item in categories:
            vocab_id = item["id"] - 1
            self.class_names[vocab_id] = item["name"]
            for s in item["synonyms"]:
                words = []
                for word in self.lemmatize(s.lower().replace("_", " ")):
                    if word.startswith("("):  # "bow (weapon)": the qualifier and everything after it are dropped
                        break
                    words.append(word)
                # (a synonym that starts with its qualifier leaves the empty phrase, as in the reference; it matches nothing
                # but an empty caption)
                self.look_up[" ".join(words).replace(" - ", "-")] = vocab_id

    @classmethod
    def from_file(cls, vocab_file, lemmatize=None):
        with open(vocab_file) as f:
            data = json.load(f)
        return cls(data["categories"] if isinstance(data, dict) else data, lemmatize)

    def parse(self, sentence):
        """-> (phrases, ids) of every look-up phrase that occurs in the lemmatised lower-case sentence as whole words: in
        the middle, at the start, at the end, or as the whole sentence -- in look-up order."""
        lemma = " ".join(self.lemmatize(sentence.lower()))
        nns, ids = [], []
        for s, vocab_id in self.look_up.items():
            if f" {s} " in lemma or lemma.startswith(s + " ") or lemma.endswith(" " + s) or lemma == s:
                nns.append(s)
                ids.append(vocab_id)
        return nns, ids

    def extract_obj(self, sentences):
        """The nouns of an image's captions: unique, in first-seen order, each with the id of its last match."""
        found = {}
        for sentence in sentences:
            for n, i in zip(*self.parse(sentence)):
                found[n] = i
        return list(found), list(found.values())
