"""The generated Swagger document matches the reference's pkg/apis/v1beta1/swagger.json (a copy is kept under
tests/golden/reference):
same definitions, same (camelCase) properties per definition, same JSON types / $refs
(the reference file is read as data; no code from it runs)."""
import json
import os

from katib_amd.api import openapi

REF = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference", "pkg", "apis", "v1beta1",
                   "swagger.json")


def _kind(s):
    if "$ref" in s:
        return "ref:" + s["$ref"].rsplit("/", 1)[-1]
    if s.get("type") == "array":
        return "array[%s]" % _kind(s["items"])
    if s.get("type") == "object" and "additionalProperties" in s:
        return "map[%s]" % _kind(s["additionalProperties"])
    return s.get("type", "object")


def test_document_is_valid_swagger():
    d = openapi.document()
    assert d["swagger"] == "2.0" and d["info"]["title"] == "Katib"
    for name, body in d["definitions"].items():
        for p, s in body["properties"].items():
            if "$ref" in s:
                target = s["$ref"].rsplit("/", 1)[-1]
                assert target in d["definitions"] or target.startswith("v1."), (name, p, target)
    json.loads(openapi.dumps())


def test_parity_with_reference_swagger():
    ref = json.load(open(REF))["definitions"]
    ours = openapi.document()["definitions"]
    assert set(ref) == set(ours), (sorted(set(ref) - set(ours)), sorted(set(ours) - set(ref)))
    diffs = []
    for name, body in ref.items():
        rp, op = body.get("properties", {}), ours[name]["properties"]
        if set(rp) != set(op):
            diffs.append((name, "props", sorted(set(rp) ^ set(op))))
            continue
        for p, s in rp.items():
            a, b = _kind(s), _kind(op[p])
            # the reference types resourceVersion-style free-form fields (trialSpec, customCollector,
            # list metadata) as k8s types we render as free-form objects
            if a != b and not (b == "object" and (a.startswith("ref:v1.") or a.startswith("ref:runtime."))):
                diffs.append((name, p, a, b))
    assert not diffs, diffs


def test_openapi_cli_and_http(tmp_path):
    import io
    import contextlib
    import urllib.request

    from katib_amd import cli
    from katib_amd.controller.apiserver import ApiServer
    from katib_amd.controller.manager import Manager

    buf = io.StringIO()
    with contextlib.redirect_stdout(buf):
        cli.main(["openapi"])
    assert "v1beta1.ExperimentSpec" in json.loads(buf.getvalue())["definitions"]
    m = Manager(state_dir=str(tmp_path), num_devices=0, journal=False)
    srv = ApiServer(m, port=0)
    srv.start()
    try:
        body = urllib.request.urlopen("http://127.0.0.1:%d/openapi/v2" % srv.port, timeout=10).read()
        d = json.loads(body)
        assert "v1.Time" in d["definitions"] and ".v1beta1.Trial" in d["definitions"]
    finally:
        srv.stop()
        m.shutdown()
