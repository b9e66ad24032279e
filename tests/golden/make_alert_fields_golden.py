#!/usr/bin/env python
"""The field lists of the reference's alert schemas as a fixture: ``alert_fields.json``.

Run once, where the reference is at hand (it does not travel with this repository):

    python tests/golden/make_alert_fields_golden.py REFERENCE_ROOT

Reads ``zuds/alert_schemas/{schema_single,schema_stack}/{alert,candidate,light_curve}.avsc`` and keeps, per field,
``{name, type, nullable}`` and nothing else: no documentation strings, no defaults, no schema file.  ``type`` is the Avro
primitive (``int``, ``long``, ``float``, ``double``, ``string``, ``bytes``), ``record`` for the nested candidate and
``array`` for the light curve; ``nullable`` says that the field's union admits ``null``.  Tests read only the JSON."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
KINDS = ('schema_single', 'schema_stack')
RECORDS = ('alert', 'candidate', 'light_curve')
PRIMITIVES = ('int', 'long', 'float', 'double', 'string', 'bytes', 'boolean')


def kind_of(t):
    if isinstance(t, dict):
        return t['type']                                  # {'type': 'array', ...}
    if t in PRIMITIVES:
        return t
    return 'record'                                       # a named record (ztf.alert.candidate)


def field(f):
    t = f['type']
    members = t if isinstance(t, list) else [t]
    rest = [m for m in members if m != 'null']
    if len(rest) != 1:
        raise ValueError(f'{f["name"]}: a union of {members}')
    return {'name': f['name'], 'type': kind_of(rest[0]), 'nullable': len(rest) != len(members)}


def main():
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    ref = sys.argv[1]
    out = {}
    for kind in KINDS:
        out[kind] = {}
        for rec in RECORDS:
            with open(os.path.join(ref, 'zuds', 'alert_schemas', kind, rec + '.avsc')) as f:
                out[kind][rec] = sorted((field(x) for x in json.load(f)['fields']), key=lambda x: x['name'])
    path = os.path.join(HERE, 'alert_fields.json')
    with open(path, 'w') as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write('\n')
    print(path, {k: {r: len(v) for r, v in d.items()} for k, d in out.items()})


if __name__ == '__main__':
    main()
