"""In-kernel s_memtime stamps of K12's row-tiled fwd_bwd kernel (diagnostic build: bash tools/build_stamps.sh, or
bash tools/build_variant.sh <name> -DPPOAF_STAMPS [-DPPOAF_STAMP_BLOCK=4 for a critic workgroup] and PPOAF_LIB=tools/libppoaf_hip_<name>.so):
shader-clock cycles per phase of one workgroup.  CRITIC_H=256 gives the C3 / C4 critic shape.  Note: a stamp is a global
store, and the backend drains vmcnt before the loads that follow it -- the phase after a stamp includes that drain."""
import sys, os, ctypes as C; sys.path.insert(0,'.')
import numpy as np, torch
from ppo_and_friends_amd import _lib
_lib.LIB_PATH=os.path.abspath(os.environ.get('PPOAF_LIB','tools/libppoaf_hip_stamps.so'))
from ppo_and_friends_amd.ppo import PPO, PermutationLoader
from ppo_and_friends_amd.environments.synthetic import SyntheticFixedLengthEnv
from ppo_and_friends_amd.spaces import Box, Discrete
import os
dev=torch.device('cuda',0); E,T,O=4096,128,4
CH=int(os.environ.get('CRITIC_H','128'))
env_gen=lambda: SyntheticFixedLengthEnv(E,O,Discrete(2),T,dev)
sp=Box(-np.inf,np.inf,(O,),np.float32)
ppo=PPO(env_gen,{"p":(None,sp,sp,Discrete(2),dict(critic_kw_args=dict(hidden_size=CH)))},device=dev,random_seed=1,normalize_obs=False,normalize_rewards=False,envs_per_proc=E,ts_per_rollout=T,batch_size=256,epochs_per_iter=1,use_graphs=False)
ppo.rollout(); pol=ppo.policies["p"]
loader=PermutationLoader(pol.dataset,256,ppo.loader_generator)
f=ppo._fused_updater("p",256); f.begin_epoch(loader.epoch_permutation())
args=f._args_for(256)
for _ in range(50): f._one(args)
torch.cuda.synchronize()
lib=_lib.load(); buf=(C.c_ulonglong*32)(); lib.ppoaf_debug_read_stamps.argtypes=[C.c_void_p]; print(lib.ppoaf_debug_read_stamps(buf))
# the lean kernel (csrc/ppo_update_lean.hip) stamps into its own translation unit's buffers: read those where it ran
form=C.c_int32(0)
lean=hasattr(lib,'ppoaf_debug_read_lean_stamps') and lib.ppoaf_ppo_update_fwd_bwd_form(C.byref(args),C.byref(form))==0 and form.value==1
print("fwd_bwd form:", "lean" if lean else "general")
if lean: lib.ppoaf_debug_read_lean_stamps.argtypes=[C.c_void_p]; lib.ppoaf_debug_read_lean_stamps(buf)
st=np.array(list(buf),dtype=np.int64).reshape(2,16)
names=["P0 idx/stats","P1 gatherX","P2 layer0","P3 hidden fwd","P4 out","P5 head","P6 out bwd","P7 hidden bwd","P8 layer0 bwd"]
d=np.diff(st[0,:10]); print("net",int(os.environ.get('STAMP_NET','0')),"total cycles",st[0,9]-st[0,0])
for n,x in zip(names,d): print("   %-16s %7d"%(n,x))
if st[0,11]: print("   first bwd layer: dgrad %d, wgrad %d, bias sums %d, barrier %d"%(st[0,10]-st[0,7], st[0,11]-st[0,10], st[0,12]-st[0,11], st[0,13]-st[0,12]))
else: print("   first bwd layer: dgrad %d, barrier %d"%(st[0,10]-st[0,7], st[0,13]-st[0,12]))      # split-wgrad chain: no wgrad here
# per-wave stamps (PPOAF_STAMP_W, second row): inside the head (from P5's start) and the output backward (from P6's start);
# side work = the output layer's gradients (wave 0) and the loss partials (wave 7), from the barrier that releases P7
w=st[1]; rel=lambda a,b: int(a-b) if a else -1
print("   P5: sDOut written %d, partials stored %d (of %d)"%(rel(w[0],st[0,5]), rel(w[1],st[0,5]), st[0,6]-st[0,5]))
print("   P6: at the barrier: wave 0 (dW_out) %d, wave 4 (db_out) %d, wave 5 %d (of %d)"%(rel(w[2],st[0,6]), rel(w[3],st[0,6]), rel(w[4],st[0,6]), st[0,7]-st[0,6]))
print("   end of the body (from the last panel copy): dW_out stored %d, partials stored %d"%(rel(w[5],w[6]) if w[6] else -1, rel(w[1],w[6]) if w[6] else -1))
# the hidden forward layers, per wave (PPOAF_HSTAMP: every wave of the stamped workgroup reads the clock in place and stores
# it behind the layer's barrier), cycles from the wave's own start of the layer: its last MFMA issued (the first dgrad load
# follows it where the layer requests a whole set), the layer's last dgrad load issued (the same stamp where it requests none),
# the last epilogue ds_write / panel store issued, the barrier passed.  "burst" = first to last load issued where the set is
# one burst; "late" = the wave's arrival at the barrier after the first wave's.  HIDDEN_WAVES picks the waves (default 0,3,7).
if hasattr(lib,'ppoaf_debug_read_hidden_stamps'):
    rd=lib.ppoaf_debug_read_lean_hidden_stamps if lean else lib.ppoaf_debug_read_hidden_stamps
    hb=(C.c_ulonglong*128)(); rd.argtypes=[C.c_void_p]; rd(hb)
    hs=np.array(list(hb),dtype=np.int64).reshape(2,8,8)
    waves=[int(x) for x in os.environ.get('HIDDEN_WAVES','0,3,7').split(',')]
    for l in range(2):
        live=[w_ for w_ in range(8) if hs[l,w_,0]]
        if not live: continue
        t0=min(hs[l,w_,0] for w_ in live); arrive={w_:max(hs[l,w_,2],hs[l,w_,3]) for w_ in live}; first=min(arrive.values())
        print("   hidden forward layer %d: all waves past the barrier %d after the first wave's start; last arrival wave %d"%(
            l+1, max(hs[l,w_,4] for w_ in live)-t0, max(arrive,key=arrive.get)))
        for w_ in waves:
            if w_ not in live: continue
            s=hs[l,w_]
            print("      wave %d: start +%d | last MFMA %d, last load %d (burst %d), epilogue written %d, barrier passed %d | late %d"%(
                w_, s[0]-t0, s[1]-s[0], s[2]-s[0], s[2]-s[1] if s[2]<s[3] else s[2]-s[3], s[3]-s[0], s[4]-s[0], arrive[w_]-first))
