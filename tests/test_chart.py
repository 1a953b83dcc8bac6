"""T-chart / T-cloudinit: offline rendering of the Helm chart.

Resource names must equal the reference's for replica 0;
new knobs (replicas, GPU passthrough, storage, eviction) render as designed; the
cloud-init scripts are executed against a fake root.
"""
import base64
import json
import os
import subprocess

import pytest
import yaml

from kvedge_amd.deploy.gotemplate import Renderer, TemplateError
from kvedge_amd.deploy.helm import Chart, apply_sets, manifests

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHART = os.path.join(ROOT, "deploy", "helm")
A1 = {  # SURVEY.md Appendix A.1, nameOverride=aziot-edge-kubevirt
    ("Secret", "aziot-edge-kubevirt-vm-aziotedgeconfig"),
    ("Secret", "aziot-edge-kubevirt-vm-cloudconfig"),
    ("DataVolume", "aziot-edge-kubevirt-linux-dv"),
    ("VirtualMachine", "aziot-edge-kubevirt-linux"),
    ("Service", "aziot-edge-kubevirt-vm-ssh-service"),
}
CFG = '[provisioning]\nsource = "manual"\nconnection_string = "HostName=x;DeviceId=y;SharedAccessKey=z"\n'


def render(sets=(), set_strings=(), files=(), name="rel"):
    ch = Chart(CHART)
    out = ch.render(name, sets=list(sets), set_strings=list(set_strings), set_files=list(files))
    return out, manifests(out)


def by_kind(objs, kind):
    return [o for o in objs if o["kind"] == kind]


@pytest.fixture
def cfg_file(tmp_path):
    p = tmp_path / "config.toml"
    p.write_text(CFG)
    return str(p)


def test_renderer_typed_eq_on_minimal_chart(tmp_path):
    """The renderer on a chart that guards a Service the way the reference's does
    (``eq <value> true``): names come through a named template, a
    bool true renders the Service, a STRING "true" does not."""
    (tmp_path / "templates").mkdir()
    (tmp_path / "Chart.yaml").write_text("apiVersion: v2\nname: mini\nversion: 0.1.0\n")
    (tmp_path / "values.yaml").write_text(
        "nameOverride: aziot-edge-kubevirt\nexternalSsh: false\npublicSshKey: ''\n")
    (tmp_path / "templates" / "_names.tpl").write_text(
        '{{- define "mini.name" -}}{{ default .Chart.Name .Values.nameOverride }}{{- end }}\n')
    (tmp_path / "templates" / "secret.yaml").write_text(
        'apiVersion: v1\nkind: Secret\nmetadata:\n  name: {{ include "mini.name" . }}-vm-cloudconfig\n'
        'stringData:\n  key: {{ .Values.publicSshKey | quote }}\n')
    (tmp_path / "templates" / "service.yaml").write_text(
        '{{- if eq .Values.externalSsh true }}\napiVersion: v1\nkind: Service\nmetadata:\n'
        '  name: {{ include "mini.name" . }}-vm-ssh-service\n{{- end }}\n')
    (tmp_path / "templates" / "NOTES.txt").write_text(
        'kubectl get vmi {{ include "mini.name" . }}-linux\n')
    ch = Chart(str(tmp_path))
    out = ch.render("chart-1634218954", sets=["publicSshKey=k,externalSsh=true"])
    objs = manifests(out)
    assert {(o["kind"], o["metadata"]["name"]) for o in objs} == {
        ("Secret", "aziot-edge-kubevirt-vm-cloudconfig"),
        ("Service", "aziot-edge-kubevirt-vm-ssh-service")}
    assert by_kind(objs, "Secret")[0]["stringData"]["key"] == "k"
    out2 = ch.render("r", set_strings=["externalSsh=true"])
    assert not by_kind(manifests(out2), "Service")
    assert by_kind(manifests(ch.render("r")), "Service") == []
    assert "kubectl get vmi aziot-edge-kubevirt-linux" in out["NOTES.txt"]


def test_default_render_keeps_reference_names(cfg_file):
    out, objs = render(sets=["publicSshKey=ssh-ed25519 AAAA"], files=["azIotEdgeConfig=" + cfg_file])
    names = {(o["kind"], o["metadata"]["name"]) for o in objs if o["kind"] != "ConfigMap"}
    assert names == A1
    vm = by_kind(objs, "VirtualMachine")[0]
    assert vm["apiVersion"] == "kubevirt.io/v1"
    assert vm["spec"]["runStrategy"] == "Always"
    labels = vm["spec"]["template"]["metadata"]["labels"]
    assert labels["kubevirt.io/domain"] == "aziot-edge-kubevirt-vm"
    assert labels["app.kubernetes.io/version"] == "0.2.0"
    assert labels["app.kubernetes.io/managed-by"] == "Helm"
    assert labels["helm.sh/chart"] == "aziot-edge-kubevirt-0.2.0"
    svc = by_kind(objs, "Service")[0]
    assert svc["spec"]["selector"]["kubevirt.io/domain"] == labels["kubevirt.io/domain"]
    assert svc["spec"]["type"] == "LoadBalancer" and svc["spec"]["ports"][0]["port"] == 22
    dv = by_kind(objs, "DataVolume")[0]
    assert dv["spec"]["pvc"]["resources"]["requests"]["storage"] == "40Gi"
    assert dv["spec"]["source"]["registry"]["url"].startswith("docker://")
    assert vm["spec"]["template"]["spec"]["volumes"][0]["dataVolume"]["name"] == dv["metadata"]["name"]
    iface = vm["spec"]["template"]["spec"]["domain"]["devices"]["interfaces"][0]
    assert iface["macAddress"] == "fe:7e:48:a0:7d:22" and "masquerade" in iface


def test_config_secret_roundtrip(cfg_file):
    _, objs = render(files=["azIotEdgeConfig=" + cfg_file])
    sec = [o for o in by_kind(objs, "Secret") if o["metadata"]["name"].endswith("aziotedgeconfig")][0]
    assert base64.b64decode(sec["data"]["userdata"]).decode() == CFG


def _cloudinit(objs, i=0):
    sec = [o for o in by_kind(objs, "Secret") if "cloudconfig" in o["metadata"]["name"]][i]
    txt = base64.b64decode(sec["data"]["userdata"]).decode()
    return txt, yaml.safe_load(txt)


def test_cloudinit_contract():
    _, objs = render(sets=["publicSshKey=ssh-ed25519 KEY"])
    txt, ci = _cloudinit(objs)
    assert txt.startswith("#cloud-config\n")
    assert ci["hostname"] == "iotedgevm" and ci["ssh_authorized_keys"] == ["ssh-ed25519 KEY"]
    vm = by_kind(objs, "VirtualMachine")[0]
    serial = [d for d in vm["spec"]["template"]["spec"]["domain"]["devices"]["disks"]
              if d["name"] == "aziotedgeconfigdisk"][0]["serial"]
    assert serial == "D23YZ9W6WA5DJ487"
    assert any(serial in " ".join(map(str, c)) for c in ci["bootcmd"])
    paths = {f["path"] for f in ci["write_files"]}
    assert "/usr/local/sbin/kvedge-apply-config" in paths
    assert "apt" not in ci  # pre-baked image: nothing to install at boot
    flat = [" ".join(map(str, c)) if isinstance(c, list) else c for c in ci["runcmd"]]
    assert any("enable --now kvedge-config.service" in c for c in flat)
    # the GPU check is a per-boot systemd oneshot, not a once-per-
    # instance runcmd line
    assert any("enable --now kvedge-gpu.service" in c for c in flat)
    assert not any("kvedge-gpu-check" in c for c in flat)
    unit = files_of(ci)["/etc/systemd/system/kvedge-gpu.service"]
    assert "ExecStart=/usr/local/sbin/kvedge-gpu-check 1 120" in unit
    assert "WantedBy=multi-user.target" in unit and "Before=aziot-edged.service" in unit
    # not pre-baked: jammy/noble Microsoft repo + installs, never bionic
    _, objs2 = render(sets=["image.prebaked=false"])
    txt2, ci2 = _cloudinit(objs2)
    assert "noble" in ci2["apt"]["sources"]["microsoft-prod.list"]["source"]
    assert "bionic" not in txt2
    assert any("aziot-edge" in " ".join(map(str, c)) for c in ci2["runcmd"])


def test_gpu_passthrough_and_firmware():
    _, objs = render(sets=["gpu.count=2"])
    spec = by_kind(objs, "VirtualMachine")[0]["spec"]["template"]
    hd = spec["spec"]["domain"]["devices"]["hostDevices"]
    assert [h["deviceName"] for h in hd] == ["amd.com/mi355x"] * 2
    assert spec["spec"]["domain"]["firmware"]["bootloader"]["efi"]["secureBoot"] is False
    ann = json.loads(spec["metadata"]["annotations"]["hooks.kubevirt.io/hookSidecars"])
    hook_cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("mmio64-hook")][0]
    assert ann[0]["configMap"]["name"] == hook_cm["metadata"]["name"]
    assert "X-PciMmio64Mb,string=1048576" in hook_cm["data"]["hook.sh"]
    assert spec["spec"]["evictionStrategy"] == "None"  # VFIO: no live migration
    # CPU-only VM (BASELINE config 1): no host devices, no hook
    _, objs0 = render(sets=["gpu.count=0"])
    spec0 = by_kind(objs0, "VirtualMachine")[0]["spec"]["template"]
    assert "hostDevices" not in spec0["spec"]["domain"]["devices"]
    assert "annotations" not in spec0["metadata"]
    assert not [o for o in by_kind(objs0, "ConfigMap") if "mmio64" in o["metadata"]["name"]]


def test_replicas_scale_out(tmp_path):
    cfgs = []
    for i in range(3):
        p = tmp_path / f"c{i}.toml"
        p.write_text(f"device = {i}\n")
        cfgs.append(str(p))
    _, objs = render(sets=["replicas=3", "macAddresses[1]=fe:7e:48:a0:7d:23"],
                     files=[f"replicaConfigs[{i}]={c}" for i, c in enumerate(cfgs)])
    vms = by_kind(objs, "VirtualMachine")
    assert [v["metadata"]["name"] for v in vms] == [
        "aziot-edge-kubevirt-linux", "aziot-edge-kubevirt-linux-1", "aziot-edge-kubevirt-linux-2"]
    svcs = by_kind(objs, "Service")
    for vm, svc in zip(vms, svcs):
        assert svc["spec"]["selector"]["kubevirt.io/domain"] == \
            vm["spec"]["template"]["metadata"]["labels"]["kubevirt.io/domain"]
    secrets = [o for o in by_kind(objs, "Secret") if "aziotedgeconfig" in o["metadata"]["name"]]
    assert [base64.b64decode(s["data"]["userdata"]).decode() for s in secrets] == \
        [f"device = {i}\n" for i in range(3)]
    assert len(by_kind(objs, "DataVolume")) == 3
    macs = [v["spec"]["template"]["spec"]["domain"]["devices"]["interfaces"][0].get("macAddress")
            for v in vms]
    assert macs[1] == "fe:7e:48:a0:7d:23" and macs[2] is None
    hosts = [_cloudinit(objs, i)[1]["hostname"] for i in range(3)]
    assert hosts == ["iotedgevm", "iotedgevm-1", "iotedgevm-2"]


def test_ssh_flag_accepts_strings_and_bools():
    for v, want in (("true", 1), ("false", 0)):
        _, a = render(set_strings=[f"aziotEdgeVmEnableExternalSsh={v}"])
        _, b = render(sets=[f"aziotEdgeVmEnableExternalSsh={v}"])
        assert len(by_kind(a, "Service")) == want and len(by_kind(b, "Service")) == want


def test_names_truncation_and_empty_override():
    long = "a" * 39 + "-bbbbbbbb"
    _, objs = render(sets=[f"nameOverride={long}"])
    vm = by_kind(objs, "VirtualMachine")[0]
    assert vm["metadata"]["name"] == "a" * 39 + "-linux"
    _, objs = render(set_strings=["nameOverride="])
    names = {o["metadata"]["name"] for o in objs}
    assert "aziot-edge-kubevirt-vm-cloudconfig" in names  # fixed quirk A.2#2
    assert not any(n.startswith("-") for n in names)


def test_storage_and_http_source():
    _, objs = render(sets=["storage.accessMode=ReadWriteMany", "storage.className=ceph-rbd",
                           "image.source=http", "image.httpUrl=https://example/img.qcow2"])
    dv = by_kind(objs, "DataVolume")[0]["spec"]
    assert dv["pvc"]["accessModes"] == ["ReadWriteMany"]
    assert dv["pvc"]["storageClassName"] == "ceph-rbd"
    assert dv["source"]["http"]["url"] == "https://example/img.qcow2"
    with pytest.raises(TemplateError, match="httpUrl"):
        render(sets=["image.source=http"])


def test_module_deployment_manifest():
    _, objs = render(sets=["module.model=yolov8n", "module.batch=32"])
    cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
    man = json.loads(cm["data"]["deployment.json"])["modulesContent"]
    mod = man["$edgeAgent"]["properties.desired"]["modules"]["kvedge"]
    co = json.loads(mod["settings"]["createOptions"])
    devs = {d["PathOnHost"] for d in co["HostConfig"]["Devices"]}
    assert devs == {"/dev/kfd", "/dev/dri"} and set(co["HostConfig"]["GroupAdd"]) == {"video", "render"}
    assert man["kvedge"]["properties.desired"]["model"] == "yolov8n"
    assert man["kvedge"]["properties.desired"]["batch"] == 32
    assert "FROM /messages/modules/kvedge/outputs/*" in \
        man["$edgeHub"]["properties.desired"]["routes"]["telemetryToCloud"]


def test_golden_default_render():
    out, _ = render(name="golden")
    got = "".join(f"---\n# {k}\n{v.strip()}\n" for k, v in sorted(out.items()))
    golden = os.path.join(CHART, "tests", "golden_default.yaml")
    if os.environ.get("KVEDGE_UPDATE_GOLDEN"):
        os.makedirs(os.path.dirname(golden), exist_ok=True)
        open(golden, "w").write(got)
    assert got == open(golden).read()


def test_set_parsing():
    v = apply_sets({"a": {"b": 1}}, sets=["a.c=true,x=3,s=str", "l[1]=z", r"k\.dot=1"],
                   set_strings=["n=007"])
    assert v == {"a": {"b": 1, "c": True}, "x": 3, "s": "str", "l": [None, "z"], "k.dot": 1,
                 "n": "007"}


def test_template_language_subset():
    r = Renderer()
    src = ('{{- define "t" -}}[{{ . }}]{{- end -}}'
           '{{ $x := 3 }}{{ range $i, $v := list "a" "b" }}{{ $i }}={{ $v }};{{ end }}'
           '{{ if and (gt $x 2) (not false) }}yes{{ else }}no{{ end }} '
           '{{ include "t" "q" | upper }} {{ printf "%s-%d" "n" 7 }} {{ "abc" | trunc 2 }} '
           '{{ with .m }}{{ .k }}{{ end }} {{ toJson (dict "b" 1 "a" (list 1 2)) }}')
    assert r.render(src, {"m": {"k": "K"}}) == '0=a;1=b;yes [Q] n-7 ab K {"a":[1,2],"b":1}'
    with pytest.raises(TemplateError):
        r.render("{{ eq 1 \"1\" }}", {})


def files_of(ci):
    return {f["path"]: f["content"] for f in ci["write_files"]}


def _fake_root_script(script: str, root) -> str:
    return (script.replace("/mnt/app-secret", f"{root}/mnt/app-secret")
            .replace("/etc/aziot", f"{root}/etc/aziot")
            .replace("/var/lib/kvedge", f"{root}/var/lib/kvedge")
            .replace("/usr/local/sbin/kvedge-stamp", f"{root}/stamp")
            .replace("/dev/kfd", f"{root}/dev/kfd").replace("/dev/dri", f"{root}/dev/dri")
            .replace("/proc/sys/kernel/random/boot_id", f"{root}/boot_id"))


def test_cloudinit_scripts_in_fake_root(tmp_path):
    _, objs = render()
    _, ci = _cloudinit(objs)
    files = {f["path"]: f["content"] for f in ci["write_files"]}
    root = tmp_path
    for d in ("mnt/app-secret", "etc", "var/lib/kvedge", "bin", "dev/dri"):
        (root / d).mkdir(parents=True, exist_ok=True)
    (root / "stamp").write_text(_fake_root_script(files["/usr/local/sbin/kvedge-stamp"], root))
    (root / "stamp").chmod(0o755)
    log = root / "iotedge.log"
    fail_flag = root / "apply-fails"
    (root / "bin" / "iotedge").write_text(
        f"#!/bin/sh\necho \"$@\" >> {log}\n"
        f"[ \"$1 $2\" = \"config apply\" ] && [ -e {fail_flag} ] && exit 3\nexit 0\n")
    (root / "bin" / "iotedge").chmod(0o755)
    apply = root / "apply.sh"
    apply.write_text(_fake_root_script(files["/usr/local/sbin/kvedge-apply-config"], root))
    env = dict(os.environ, PATH=f"{root}/bin:" + os.environ["PATH"])
    run = lambda: subprocess.run(["sh", str(apply)], env=env, capture_output=True)  # noqa
    assert run().returncode == 0  # no config on the disk: nothing happens
    assert not log.exists()
    (root / "mnt/app-secret/userdata").write_text(CFG)
    # a failed `iotedge config apply` must not leave a config.toml that
    # makes every later boot skip the apply
    fail_flag.write_text("")
    assert run().returncode == 1
    assert not (root / "etc/aziot/config.toml").exists()
    fail_flag.unlink()
    assert run().returncode == 0
    assert (root / "etc/aziot/config.toml").read_text() == CFG
    assert log.read_text().count("config apply") == 2
    assert run().returncode == 0  # unchanged: idempotent, no re-apply
    assert log.read_text().count("config apply") == 2
    (root / "mnt/app-secret/userdata").write_text(CFG + "# rotated\n")
    assert run().returncode == 0
    assert log.read_text().count("config apply") == 3
    assert (root / "etc/aziot/config.toml").read_text().endswith("# rotated\n")
    # GPU check: times out without devices, succeeds once /dev/kfd + a render node exist
    gpu = root / "gpu.sh"
    gpu.write_text(_fake_root_script(files["/usr/local/sbin/kvedge-gpu-check"], root))
    (root / "boot_id").write_text("boot-A\n")
    r = subprocess.run(["sh", str(gpu), "1", "1"], capture_output=True)
    assert r.returncode == 1
    assert json.loads((root / "var/lib/kvedge/gpu.json").read_text())["error"] == "timeout"
    assert "gpu_missing" in (root / "var/lib/kvedge/boot-timing").read_text()
    (root / "dev/kfd").write_text("")
    (root / "dev/dri/renderD128").write_text("")
    r = subprocess.run(["sh", str(gpu), "1", "2"], capture_output=True)
    assert r.returncode == 0
    info = json.loads((root / "var/lib/kvedge/gpu.json").read_text())
    assert info["kfd"] is True and info["render_nodes"] == 1 and info["boot_id"] == "boot-A"
    stamps = (root / "var/lib/kvedge/boot-timing").read_text()
    assert "config_applied" in stamps and "gpu_ready" in stamps


def _fake_iotedge(root, agent_after: int, check_after: int):
    """`iotedge` stand-in: edgeAgent shows as running from the agent_after-th `list`
    call on, `check` passes from the check_after-th call on."""
    (root / "bin").mkdir(parents=True, exist_ok=True)
    n = root / "calls"
    (root / "bin" / "iotedge").write_text(f"""#!/bin/sh
c=$(cat {n}.$1 2>/dev/null || echo 0); c=$((c+1)); echo $c > {n}.$1
if [ "$1" = list ]; then
  echo "NAME STATUS DESCRIPTION CONFIG"
  [ $c -ge {agent_after} ] && echo "edgeAgent running Up 3 seconds mcr.microsoft.com/azureiotedge-agent:1.5"
  exit 0
fi
if [ "$1" = check ]; then
  [ $c -ge {check_after} ] && {{ echo '{{"checks": {{}}, "result": "ok"}}'; exit 0; }}
  echo '{{"result": "failed"}}'; exit 1
fi
""")
    (root / "bin" / "iotedge").chmod(0o755)


def test_ready_service_stamps_iotedge_check(tmp_path):
    """the guest stamps edge_agent_running and iotedge_check_pass (the
    boot-to-ready end point) from a bounded poll, and the collector turns the stamps into
    boot_to_ready_s."""
    _, objs = render()
    _, ci = _cloudinit(objs)
    files = {f["path"]: f["content"] for f in ci["write_files"]}
    assert "kvedge-ready 900 2" in files["/etc/systemd/system/kvedge-ready.service"]
    assert "After=kvedge-config.service" in files["/etc/systemd/system/kvedge-ready.service"]
    flat = [" ".join(map(str, c)) for c in ci["runcmd"]]
    assert any("enable --now --no-block kvedge-ready.service" in c for c in flat)
    root = tmp_path
    (root / "var/lib/kvedge").mkdir(parents=True)
    (root / "stamp").write_text(_fake_root_script(files["/usr/local/sbin/kvedge-stamp"], root))
    (root / "stamp").chmod(0o755)
    ready = root / "ready.sh"
    ready.write_text(_fake_root_script(files["/usr/local/sbin/kvedge-ready"], root))
    _fake_iotedge(root, agent_after=2, check_after=3)
    env = dict(os.environ, PATH=f"{root}/bin:" + os.environ["PATH"])
    r = subprocess.run(["sh", str(ready), "30", "0"], env=env, capture_output=True)
    assert r.returncode == 0, r.stderr
    from kvedge_amd.utils.boottime import parse_stamps

    st = parse_stamps((root / "var/lib/kvedge/boot-timing").read_text())
    assert st["edge_agent_running"] <= st["iotedge_check_pass"]
    assert json.loads((root / "var/lib/kvedge/iotedge-check.json").read_text())["result"] == "ok"
    # a check that never passes ends bounded, with a timeout stamp
    root2 = tmp_path / "r2"
    (root2 / "var/lib/kvedge").mkdir(parents=True)
    (root2 / "stamp").write_text(_fake_root_script(files["/usr/local/sbin/kvedge-stamp"], root2))
    (root2 / "stamp").chmod(0o755)
    ready2 = root2 / "ready.sh"
    ready2.write_text(_fake_root_script(files["/usr/local/sbin/kvedge-ready"], root2))
    _fake_iotedge(root2, agent_after=1, check_after=10 ** 6)
    env2 = dict(os.environ, PATH=f"{root2}/bin:" + os.environ["PATH"])
    r = subprocess.run(["sh", str(ready2), "1", "0"], env=env2, capture_output=True)
    assert r.returncode == 1
    txt = (root2 / "var/lib/kvedge/boot-timing").read_text()
    assert "iotedge_check_timeout" in txt and "iotedge_check_pass" not in txt


def test_empty_ssh_key_renders_no_authorized_keys():
    _, objs = render()
    txt, ci = _cloudinit(objs)
    assert "ssh_authorized_keys" not in ci and "null" not in txt.split("bootcmd")[0]


def test_multi_vm_dp_wiring():
    """VERDICT r1 #3 (BASELINE config 3): replicas=4 one-GPU VMs -> rendezvous Service on
    replica 0, bridge-bound NICs, one deployment manifest per VM with its rank env and
    RCCL socket settings; replicas=1 keeps the reference's masquerade contract."""
    _, objs = render(sets=["replicas=4"], name="rel")
    rdzv = [o for o in by_kind(objs, "Service") if o["metadata"]["name"].endswith("dp-rendezvous")]
    assert len(rdzv) == 1
    assert rdzv[0]["spec"]["clusterIP"] == "None"
    assert rdzv[0]["spec"]["selector"] == {"kubevirt.io/domain": "aziot-edge-kubevirt-vm"}
    assert rdzv[0]["spec"]["ports"][0]["port"] == 29500
    vms = by_kind(objs, "VirtualMachine")
    for vm in vms:
        iface = vm["spec"]["template"]["spec"]["domain"]["devices"]["interfaces"][0]
        assert "bridge" in iface and "masquerade" not in iface
    cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
    keys = sorted(cm["data"])
    assert keys == ["deployment-1.json", "deployment-2.json", "deployment-3.json", "deployment.json"]
    for i, k in enumerate(["deployment.json", "deployment-1.json", "deployment-2.json",
                           "deployment-3.json"]):
        man = json.loads(cm["data"][k])["modulesContent"]
        mod = man["$edgeAgent"]["properties.desired"]["modules"]["kvedge"]
        env = {k2: v["value"] for k2, v in mod["env"].items()}
        assert env["KVEDGE_NODE_RANK"] == str(i) and env["KVEDGE_NNODES"] == "4"
        assert env["KVEDGE_RANKS_PER_NODE"] == "1" and env["MASTER_PORT"] == "29500"
        assert env["MASTER_ADDR"] == "aziot-edge-kubevirt-dp-rendezvous.default.svc.cluster.local"
        assert env["NCCL_IB_DISABLE"] == "1" and env["NCCL_SOCKET_IFNAME"].startswith("^lo")
        co = json.loads(mod["settings"]["createOptions"])["HostConfig"]
        assert co["NetworkMode"] == "host"
        assert "/var/lib/kvedge:/var/lib/kvedge" in co["Binds"]
        assert man["kvedge"]["properties.desired"]["world_size"] == 4
    # topology (a): one VM, 8 GPUs -> 8 local ranks, no rendezvous Service, masquerade kept
    _, objs = render(sets=["gpu.count=8"])
    assert not [o for o in by_kind(objs, "Service") if "rendezvous" in o["metadata"]["name"]]
    iface = by_kind(objs, "VirtualMachine")[0]["spec"]["template"]["spec"]["domain"]["devices"]["interfaces"][0]
    assert "masquerade" in iface
    cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
    mod = json.loads(cm["data"]["deployment.json"])["modulesContent"]["$edgeAgent"][
        "properties.desired"]["modules"]["kvedge"]
    env = {k2: v["value"] for k2, v in mod["env"].items()}
    assert env["KVEDGE_RANKS_PER_NODE"] == "8" and env["MASTER_ADDR"] == "127.0.0.1"
    assert "NetworkMode" not in json.loads(mod["settings"]["createOptions"])["HostConfig"]


def _module_envs(objs):
    cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
    out = []
    for k in sorted(cm["data"], key=lambda k: (k != "deployment.json", k)):  # replica order
        man = json.loads(cm["data"][k])["modulesContent"]
        mod = man["$edgeAgent"]["properties.desired"]["modules"]["kvedge"]
        out.append(({k2: v["value"] for k2, v in mod["env"].items()},
                    man["kvedge"]["properties.desired"]["world_size"]))
    return out


def test_dp_disabled_replicas_are_independent_jobs():
    """with dp.enabled=false the replicas are independent devices.  No
    VM may get cross-VM rank env (which would make each module rendezvous as rank i of a
    world-N job on its own loopback and hang)."""
    _, objs = render(sets=["replicas=2", "dp.enabled=false"])
    assert not [o for o in by_kind(objs, "Service") if "rendezvous" in o["metadata"]["name"]]
    envs = _module_envs(objs)
    assert len(envs) == 2
    for env, world in envs:
        assert "KVEDGE_NODE_RANK" not in env and "KVEDGE_NNODES" not in env
        assert "MASTER_ADDR" not in env and world == 1
    # 2 VMs x 4 GPUs, DP off: each VM runs its own 4-rank job on loopback
    _, objs = render(sets=["replicas=2", "dp.enabled=false", "gpu.count=4"])
    for env, world in _module_envs(objs):
        assert env["KVEDGE_NODE_RANK"] == "0" and env["KVEDGE_NNODES"] == "1"
        assert env["KVEDGE_RANKS_PER_NODE"] == "4" and env["MASTER_ADDR"] == "127.0.0.1"
        assert "NCCL_SOCKET_IFNAME" not in env and world == 4
    # DP on with 2 x 4 GPUs: world 8 across VMs
    _, objs = render(sets=["replicas=2", "gpu.count=4"])
    for i, (env, world) in enumerate(_module_envs(objs)):
        assert env["KVEDGE_NODE_RANK"] == str(i) and env["KVEDGE_NNODES"] == "2" and world == 8


def test_config_toml_is_git_ignored():
    """Reference .gitignore:1-2 keeps config.toml (IoT Hub connection string) out of git."""
    pats = [ln.strip() for ln in open(os.path.join(ROOT, ".gitignore")) if ln.strip()]
    assert "*.toml" in pats
    if subprocess.run(["git", "-C", ROOT, "rev-parse"], capture_output=True).returncode == 0:
        r = subprocess.run(["git", "-C", ROOT, "check-ignore", "-q", "config.toml"])
        assert r.returncode == 0


def test_guest_image_build_targets_guest_kernel():
    """DKMS under virt-customize builds for the appliance kernel unless
    told otherwise.  The build script builds amdgpu for the image's own kernel, fails the
    build if the module is missing, and pre-loads the edge runtime images (no pull at boot)."""
    p = os.path.join(ROOT, "deploy", "image", "build-disk.sh")
    txt = open(p).read()
    assert subprocess.run(["bash", "-n", p]).returncode == 0
    assert "dkms autoinstall -k \\$KVER" in txt and "modinfo -k \\$KVER amdgpu" in txt
    assert "set -euo pipefail" in txt
    assert "kvedge-preload.service" in txt and "Before=aziot-edged.service" in txt
    assert "docker save" in txt and "--copy-in build/images:/var/lib/kvedge" in txt


def test_vmi_health_probes_and_heartbeat_script(tmp_path):
    """the VM template carries guest-agent exec readiness / liveness
    probes; `kvedge-health` reads the module heartbeat the module writes (fresh -> ready,
    stale -> not live, absent -> not ready but live); the module manifest points the
    module at that file; health.enabled=false removes the probes."""
    import time

    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    _, objs = render(sets=["gpu.count=0"])  # CPU VM: the GPU evidence is the next test's
    spec = by_kind(objs, "VirtualMachine")[0]["spec"]["template"]["spec"]
    rp, lp = spec["readinessProbe"], spec["livenessProbe"]
    assert rp["exec"]["command"] == ["/usr/local/sbin/kvedge-health", "ready"]
    assert lp["exec"]["command"] == ["/usr/local/sbin/kvedge-health", "live"]
    assert rp["periodSeconds"] == 10 and lp["initialDelaySeconds"] == 600
    _, ci = _cloudinit(objs)
    flat = [" ".join(map(str, c)) if isinstance(c, list) else c for c in ci["runcmd"]]
    assert any("qemu-guest-agent" in c for c in flat)
    cm = [o for o in by_kind(objs, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
    dep = json.loads(cm["data"]["deployment.json"])
    env = dep["modulesContent"]["$edgeAgent"]["properties.desired"]["modules"]["kvedge"]["env"]
    assert env["KVEDGE_HEARTBEAT"]["value"] == "/var/lib/kvedge/heartbeat"
    # the script, in a fake root (its own boot id file)
    files = {f["path"]: f["content"] for f in ci["write_files"]}
    (tmp_path / "var/lib/kvedge").mkdir(parents=True)
    boot_id = tmp_path / "boot_id"
    boot_id.write_text("boot-A\n")
    sh = tmp_path / "health.sh"
    sh.write_text(_fake_root_script(files["/usr/local/sbin/kvedge-health"], tmp_path))
    probe = lambda what: subprocess.run(["sh", str(sh), what]).returncode  # noqa: E731
    assert probe("ready") != 0 and probe("live") == 0  # booting: no heartbeat yet
    # the module writes the heartbeat (with the boot id) from its first step on
    tr = FakeTransport({"model": "simulated-temperature", "send_interval_s": 1.0})
    hb = tmp_path / "var/lib/kvedge/heartbeat"
    app = ModuleApp(tr, device="cpu", heartbeat_path=str(hb), boot_id_path=str(boot_id)).start()
    app.run(max_steps=2)
    app.stop()
    beat = json.loads(hb.read_text())
    assert beat["model"] == "simulated-temperature" and beat["boot_id"] == "boot-A"
    assert probe("ready") == 0 and probe("live") == 0
    old = time.time() - 3600
    os.utime(hb, (old, old))  # module hung: heartbeat stale
    assert probe("ready") != 0 and probe("live") != 0
    # the VMI restarted.  The heartbeat the previous boot wrote
    # 5 s ago is fresh by age but from another boot: not ready (and live: booting)
    recent = time.time() - 5
    os.utime(hb, (recent, recent))
    boot_id.write_text("boot-B\n")
    assert probe("ready") != 0 and probe("live") == 0
    # ... until this boot's module writes its own
    app2 = ModuleApp(FakeTransport({"model": "simulated-temperature"}), device="cpu",
                     heartbeat_path=str(hb), boot_id_path=str(boot_id)).start()
    app2.run(max_steps=1)
    app2.stop()
    assert probe("ready") == 0 and probe("live") == 0
    # module disabled: readiness = THIS boot's iotedge check passed
    _, objs2 = render(sets=["module.enabled=false", "gpu.count=0"])
    _, ci2 = _cloudinit(objs2)
    f2 = {f["path"]: f["content"] for f in ci2["write_files"]}
    sh.write_text(_fake_root_script(f2["/usr/local/sbin/kvedge-health"], tmp_path))
    assert probe("ready") != 0
    stamp = tmp_path / "stamp"
    stamp.write_text(_fake_root_script(f2["/usr/local/sbin/kvedge-stamp"], tmp_path))
    bt = tmp_path / "var/lib/kvedge/boot-timing"
    # (ii) an iotedge_check_pass line from before the last bootcmd (the previous boot)
    bt.write_text("bootcmd 1.0 boot-B\niotedge_check_pass 2.0 boot-B\n")
    boot_id.write_text("boot-C\n")
    bt.write_text(bt.read_text() + "bootcmd 3.0 boot-C\n")
    assert probe("ready") != 0
    assert subprocess.run(["sh", str(stamp), "iotedge_check_pass"]).returncode == 0
    assert bt.read_text().splitlines()[-1].split()[2] == "boot-C"
    assert probe("ready") == 0
    # the stamp collector still reads every boot's lines
    from kvedge_amd.utils.boottime import parse_stamps
    st = parse_stamps(bt.read_text())
    assert "iotedge_check_pass#2" in st and "bootcmd#2" in st
    _, objs3 = render(sets=["health.enabled=false"])
    spec3 = by_kind(objs3, "VirtualMachine")[0]["spec"]["template"]["spec"]
    assert "readinessProbe" not in spec3 and "livenessProbe" not in spec3


def test_health_requires_this_boots_gpu(tmp_path):
    """VERDICT r5 next #2 (BASELINE config 5): with gpu.count > 0 a VMI is Ready only when
    THIS boot's kvedge-gpu-check stamped gpu_ready and the module's heartbeat says it
    serves on the GPU.  A module that fell back to the CPU, or a boot whose GPU never
    showed up (failed re-attach), stays not-ready."""
    import torch

    from kvedge_amd.module.app import ModuleApp
    from kvedge_amd.module.transport import FakeTransport

    _, objs = render()  # gpu.count = 1 (default)
    _, ci = _cloudinit(objs)
    files = files_of(ci)
    (tmp_path / "var/lib/kvedge").mkdir(parents=True)
    (tmp_path / "dev/dri").mkdir(parents=True)
    boot_id = tmp_path / "boot_id"
    boot_id.write_text("boot-A\n")
    for name, path in (("health.sh", "/usr/local/sbin/kvedge-health"),
                       ("gpu.sh", "/usr/local/sbin/kvedge-gpu-check"),
                       ("stamp", "/usr/local/sbin/kvedge-stamp")):
        (tmp_path / name).write_text(_fake_root_script(files[path], tmp_path))
        (tmp_path / name).chmod(0o755)
    probe = lambda: subprocess.run(["sh", str(tmp_path / "health.sh"), "ready"]).returncode  # noqa
    gpu_check = lambda: subprocess.run(["sh", str(tmp_path / "gpu.sh"), "1", "1"],  # noqa
                                       capture_output=True).returncode
    hb = tmp_path / "var/lib/kvedge/heartbeat"
    app = ModuleApp(FakeTransport({"model": "simulated-temperature"}), device="cpu",
                    heartbeat_path=str(hb), boot_id_path=str(boot_id)).start()
    app.run(max_steps=1)
    # (1) a fresh heartbeat of this boot from a module on the CPU: not ready, even with
    # this boot's gpu_ready stamp
    (tmp_path / "dev/kfd").write_text("")
    (tmp_path / "dev/dri/renderD128").write_text("")
    assert gpu_check() == 0
    assert json.loads(hb.read_text())["device"] == "cpu"
    assert probe() != 0
    # (2) the module serves on the GPU (the heartbeat writer of a cuda-device module) and
    # this boot's gpu_ready exists: ready
    app.device, app.gpus = torch.device("cuda"), 1
    app._heartbeat({})
    beat = json.loads(hb.read_text())
    assert beat["device"] == "cuda" and beat["gpus"] == 1
    assert probe() == 0
    # (3) the VMI restarted on another node and the GPU did not come back: the previous
    # boot's gpu_ready does not count, this boot's check stamps gpu_missing
    boot_id.write_text("boot-B\n")
    (tmp_path / "dev/kfd").unlink()
    app.boot_id = "boot-B"
    app._heartbeat({})  # even a (hypothetical) heartbeat claiming cuda for this boot
    assert gpu_check() == 1
    assert probe() != 0
    bt = (tmp_path / "var/lib/kvedge/boot-timing").read_text().splitlines()
    assert bt[-1].split()[0] == "gpu_missing" and bt[-1].split()[2] == "boot-B"
    # (4) the GPU appears within this boot: ready again
    (tmp_path / "dev/kfd").write_text("")
    assert gpu_check() == 0
    assert probe() == 0
    app.stop()
    # module disabled, GPU VM: this boot's iotedge check AND this boot's gpu_ready
    _, objs2 = render(sets=["module.enabled=false"])
    f2 = files_of(_cloudinit(objs2)[1])
    (tmp_path / "health.sh").write_text(_fake_root_script(f2["/usr/local/sbin/kvedge-health"], tmp_path))
    boot_id.write_text("boot-C\n")
    subprocess.run(["sh", str(tmp_path / "stamp"), "iotedge_check_pass"], check=True)
    assert probe() != 0
    assert gpu_check() == 0
    assert probe() == 0
    # the module manifest carries the GPU requirement (and not on a CPU VM)
    def mod_env(objs_):
        cm = [o for o in by_kind(objs_, "ConfigMap") if o["metadata"]["name"].endswith("module-deployment")][0]
        dep = json.loads(cm["data"]["deployment.json"])
        return dep["modulesContent"]["$edgeAgent"]["properties.desired"]["modules"]["kvedge"]["env"]
    assert mod_env(objs)["KVEDGE_REQUIRE_GPU"]["value"] == "1"
    assert "KVEDGE_REQUIRE_GPU" not in mod_env(render(sets=["gpu.count=0"])[1])
