"""A pure-Python reader of a translated construction from GFA (include/gbwt_hip.h, "construction from GFA with a node-to-segment
translation"), written from that contract and not from the library: what a built handle must hold.  Segment names become the ranks of
their S-lines, the text with those ranks as integer names goes through the reader of the untranslated grammar (gfa_expect.py: path
order, metadata and their refusals are the same), and the steps on segments are expanded to nodes."""
import re

import gfa_expect as X

NEVER, AUTO, ALWAYS = 0, 1, 2
MAX_NAME = 255


def chunks(sequence, max_node):
    if not max_node:
        return [sequence]
    return [sequence[i:i + max_node] for i in range(0, len(sequence), max_node)]


class Translated:
    """translated: whether a translation is built (else every attribute of gfa_expect.Expected is there instead).  segments: rows
    [rank, stored name, first node, past-the-end node, stored sequence] as in graph_known.json (name and sequence "" where no path goes);
    paths: rows of GBWT nodes; segment_paths: rows of 2 * rank + reverse; node_labels: {node id: bytes}; names / samples / contigs: the
    metadata as in Expected."""

    def __init__(self, text, max_node=0, translate=AUTO):
        if isinstance(text, str):
            text = text.encode()
        assert translate in (AUTO, ALWAYS)
        lines = text.split(b"\n")
        if lines and lines[-1] == b"":
            lines.pop()
        lines = [raw.decode("latin-1") for raw in lines]
        fields = [raw.split("\t") for raw in lines]
        s_lines = [(n, f) for n, f in enumerate(fields, 1) if "\r" not in lines[n - 1] and f[0] == "S" and len(f) >= 3]
        needed = any(not X._node_id(f[1]) for _, f in s_lines) or \
            (max_node > 0 and any(X._node_id(f[1]) and f[2] != "*" and len(f[2]) > max_node for _, f in s_lines))
        if translate == AUTO and not needed:
            self._plain(text)
            return

        errors, rank, self.all_segments = [], {}, []          # all_segments: (name, sequence) by rank
        canon = list(lines)
        for n, f in s_lines:
            if f[1] == "":
                errors.append((n, X.INVALID_DATA, "empty name"))
            elif len(f[1]) > MAX_NAME:
                errors.append((n, X.UNSUPPORTED, "long name"))
            elif f[2] in ("", "*"):
                errors.append((n, X.INVALID_DATA, "no sequence"))
            elif f[1] in rank:
                errors.append((n, X.INVALID_DATA, "duplicate name"))
            else:
                rank[f[1]] = len(self.all_segments)
                self.all_segments.append((f[1], f[2]))
                canon[n - 1] = f"S\t{rank[f[1]] + 1}\tA"
                continue
            canon[n - 1] = "#"

        def tokens_of(n, f):
            """[(name, reverse)] of a path line, or None after a refusal"""
            walk = f[0] == "W"
            field = f[6] if walk else f[2]
            if field in ("", "*"):
                return []
            if walk:
                tokens = re.findall(r"[<>][^<>]*", field)
                if "".join(tokens) != field or any(len(t) < 2 for t in tokens):
                    errors.append((n, X.INVALID_DATA, "walk"))
                    return None
                steps = [(t[1:], t[0] == "<") for t in tokens]
            else:
                tokens = field.split(",")
                if any(len(t) < 2 or t[-1] not in "+-" for t in tokens):
                    errors.append((n, X.INVALID_DATA, "steps"))
                    return None
                steps = [(t[:-1], t[-1] == "-") for t in tokens]
            if any(name not in rank for name, _ in steps):
                errors.append((n, X.INVALID_DATA, "unknown segment"))
                return None
            return steps

        for n, f in enumerate(fields, 1):
            if "\r" in lines[n - 1] or f[0] not in ("P", "W") or len(f) < (7 if f[0] == "W" else 3):
                continue
            steps = tokens_of(n, f)
            if steps is None:
                canon[n - 1] = "#"
            elif f[0] == "W":
                f = list(f)
                f[6] = "".join(f"{'<' if r else '>'}{rank[name] + 1}" for name, r in steps)
                canon[n - 1] = "\t".join(f)
            else:
                f = list(f)
                f[2] = ",".join(f"{rank[name] + 1}{'-' if r else '+'}" for name, r in steps)
                canon[n - 1] = "\t".join(f)
        try:
            by_rank = X.Expected("\n".join(canon).encode("latin-1") + b"\n")
        except X.Refused as e:
            errors.append((e.line, e.status, str(e)))
            by_rank = None
        if errors:
            raise X.Refused(*min(errors))
        self.samples, self.contigs, self.names, self.haplotypes = by_rank.samples, by_rank.contigs, by_rank.names, by_rank.haplotypes
        self.links, self.path_lines, self.steps, self.reference_samples = by_rank.links, by_rank.path_lines, by_rank.steps, by_rank.reference_samples
        self.segment_paths = [[v - 2 for v in row] for row in by_rank.paths]
        visited = {v // 2 for row in self.segment_paths for v in row}
        if not visited:                                       # no visits: no nodes, no translation
            self._plain(text if not needed else "\n".join(canon).encode("latin-1") + b"\n")
            return
        self.translated = True
        self.max_node = max_node
        self.segments, self.node_labels, self.nodes_of = [], {}, []
        node = 1
        for k, (name, sequence) in enumerate(self.all_segments):
            parts = chunks(sequence, max_node)
            self.nodes_of.append(range(node, node + len(parts)))
            seen = k in visited
            self.segments.append([k, name if seen else "", node, node + len(parts), sequence if seen else ""])
            for j, part in enumerate(parts):
                self.node_labels[node + j] = part.encode("latin-1") if seen else b""
            node += len(parts)
        self.total_nodes = node - 1
        self.paths = []
        for row in self.segment_paths:
            out = []
            for v in row:
                ids = self.nodes_of[v // 2]
                out.extend(2 * i + 1 for i in reversed(ids)) if v & 1 else out.extend(2 * i for i in ids)
            self.paths.append(out)

    def _plain(self, text):
        plain = X.Expected(text)
        self.__dict__.update(plain.__dict__)
        self.translated = False
        self.plain = plain
