"""The descriptor lists behind tests/golden/build_layers_cpu.json: what build_layers answered for each of them BEFORE it was cut into one function per layer family
(docs/history/build_layers.md names the commit and the command).  dqn_plan_default runs build_layers on the host, so all of it is observed without a GPU.  The fixture
holds, per case, what `observe` returned on that commit; the test calls the same function on the library under test and compares for equality.  Nothing here computes an
expected value.

REFUSALS   one case per `return fail(...)` site of build_layers, named s<site>_<what>; the sites are numbered 1 .. 116 in the order in which the function held them on that
           commit (SITES below).  Case k breaks rule k AND, where one descriptor can, the rules behind it in the same block (another stream, an unknown activation, unused
           slots set, a wrong size), so a reordering answers with another message.  Cases with a letter behind the site number (s76b_...) are further variants of the site: another noun of
           a noun chain, another sub-clause of the condition.  Every site is reachable; what is NOT reachable is two sub-clauses: in site 8 ("conv kernel/stride does
           not fit", the pad-0 Conv's) the terms `+ 2 * ph` / `+ 2 * pw` only ever see ph = pw = 0, because a padded Conv with that fault has been answered by site 7 one
           line above.  They are kept as they were (the line reads as the general formula).
ACCEPTED   a front (a list of descriptors build_layers accepts) and a tail that makes it a whole network.  Behind every prefix of the front stand, one at a time, three probe
           descriptors -- a Conv with cin = -1, a MaxPool with a 9999 window, a Dense with n_in = -1 -- whose refusals print the channels, the h x w map and the feature count
           the prefix produced; behind a dueling front a Dense probe stands in each stream.  front + tail yields the default plan at B = 8 and B = 128, which reads K, N,
           npos, kernel, stride, src and stream."""
import struct

import kind_traits_cases as K

pkg, nn, abi = K.pkg, K.nn, K.abi
D, CV, LSTM, GRU, RNN, MAXP, MEANP, LN, DO, SK = abi.LAYER_DENSE, abi.LAYER_CONV, abi.LAYER_LSTM, abi.LAYER_GRU, abi.LAYER_RNN, abi.LAYER_MAXPOOL, abi.LAYER_MEANPOOL, abi.LAYER_LAYERNORM, abi.LAYER_DROPOUT, abi.LAYER_SKIPADD
SKM, GN, AMAXP, AMEANP, ACT, CDG = abi.LAYER_SKIPADD_MAP, abi.LAYER_GROUPNORM, abi.LAYER_ADAPTIVEMAXPOOL, abi.LAYER_ADAPTIVEMEANPOOL, abi.LAYER_ACTIVATION, abi.LAYER_CONV_DG
dn, cv, pool, ln, do, sk = K.dn, K.cv, K.pool, K.ln, K.do, K.sk


def R(kind, stream=0, act=0, n_in=0, n_out=0, cin=0, cout=0, kh=0, kw=0, sh=0, sw=0):
    """a descriptor slot by slot (kind_traits_cases.desc has square kernels and strides only)"""
    d = abi.LayerDesc(); d.kind, d.act, d.stream, d.n_in, d.n_out, d.cin, d.cout, d.kh, d.kw, d.sh, d.sw = kind, act, stream, n_in, n_out, cin, cout, kh, kw, sh, sw
    return d


i32 = lambda u: struct.unpack("<i", struct.pack("<I", u & 0xffffffff))[0]      # a 32-bit pattern as the int32 a descriptor slot holds
f32 = lambda x: i32(struct.unpack("<I", struct.pack("<f", x))[0])              # the fp32 bit pattern of x (LayerNorm / GroupNorm eps)
f64 = lambda x: tuple(i32(w) for w in struct.unpack("<II", struct.pack("<d", x)))      # (cin, cout) = (low, high) word of the Float64 x (Dropout p)
pk, dg = lambda ph, pw: ph | pw << 16, lambda dh, dw, g: dh | dw << 8 | g << 16      # the packed slots of a dilated / grouped Conv
cdg = lambda ci, co, k=3, s=1, pad=(0, 0), dil=(1, 1), g=1, **kw: R(CDG, cin=ci, cout=co, kh=k, kw=k, sh=s, sw=s, n_in=pk(*pad), n_out=dg(*dil, g), **kw)
gn = lambda G=2, **kw: R(GN, kh=G, **kw)
actl = lambda a=11, **kw: R(ACT, act=a, **kw)
skm = lambda m, n=0, **kw: R(SKM, cin=m, n_in=n, n_out=n, **kw)
rec = lambda kind, a, b, **kw: R(kind, n_in=a, n_out=b, **kw)
apool = lambda oh, ow, kind=AMAXP, **kw: R(kind, kh=oh, kw=ow, **kw)

VEC, IMG = dict(obs=(6, 1, 1)), dict(obs=(2, 8, 8))
REC = VEC | dict(recurrence=1, trace_length=3)
first = lambda: dn(6, 16, act=1)
# fronts that end in a feature vector of 16, one per noun of the "what is layer prev" chain (an Activation layer on a feature vector / the join of a skip block on a feature
# vector / a recurrent layer / a LayerNorm layer / a Dropout layer / a Dense layer)
VEC_FRONTS = {"act": ([first(), actl()], VEC), "skip": ([first(), dn(16, 16), sk(1)], VEC), "rec": ([rec(LSTM, 6, 16)], REC), "ln": ([first(), ln(16)], VEC), "do": ([first(), do()], VEC),
              "dense": ([first()], VEC)}


def _refusals():
    c = {}
    # ---- 1: the layer count
    c["s1_no_layers"] = ([], VEC)
    c["s1b_33_layers"] = ([dn(6, 6) for _ in range(33)], VEC)
    # ---- 2 .. 8: Conv (pad in n_in / n_out)
    conv = lambda **kw: [R(CV, **({"cin": 2, "cout": 4, "kh": 3, "kw": 3, "sh": 0, "sw": 1, "stream": 1, "n_in": -1, "n_out": 5} | kw))]
    c["s2_conv_act"] = (conv(act=99, cin=3), IMG)
    c["s2b_conv_act_11"] = (conv(act=11, cin=3), IMG)
    c["s2c_conv_act_neg"] = (conv(act=-1, cin=3), IMG)
    c["s3_conv_cin"] = (conv(act=1, cin=3), IMG)
    c["s4_conv_pad_negative"] = (conv(), IMG)
    c["s4b_conv_pad_w_negative"] = (conv(n_in=1, n_out=-2), IMG)
    c["s5_conv_pad_above_kernel"] = (conv(n_in=5, n_out=0), IMG)
    c["s5b_conv_pad_kernel_0"] = (conv(n_in=1, n_out=0, kh=0), IMG)
    c["s5c_conv_pad_w_above_kernel"] = (conv(n_in=0, n_out=3), IMG)
    c["s6_conv_pad_stream"] = (conv(n_in=1, n_out=2), IMG)
    c["s6b_conv_pad_w_stream_adv"] = (conv(n_in=0, n_out=1, stream=2), IMG)
    c["s7_conv_pad_stride_0"] = (conv(n_in=1, n_out=2, stream=0), IMG)
    c["s7b_conv_pad_kernel_above_map"] = (conv(n_in=1, n_out=1, stream=0, kh=12, sh=1), IMG)
    c["s7c_conv_pad_kernel_w_above_map"] = (conv(n_in=0, n_out=1, stream=0, kw=11, sh=1), IMG)
    c["s7d_conv_pad_stride_w_0"] = (conv(n_in=1, n_out=0, stream=0, sh=1, sw=0), IMG)
    c["s8_conv_stride_0"] = (conv(n_in=0, n_out=0), IMG)                                        # (a pad-0 Conv may stand in a stream: no rule is broken by stream = 1)
    c["s8b_conv_kernel_above_map"] = (conv(n_in=0, n_out=0, stream=0, kh=9, sh=1), IMG)
    c["s8c_conv_after_vector"] = ([first(), R(CV, cin=16, cout=4, kh=1, kw=2, sh=1, sw=1)], VEC)      # a feature vector is a (16, 1, 1) map
    # ---- 9 .. 17: dilated / grouped Conv
    g = lambda **kw: [R(CDG, **({"cin": 3, "cout": 4, "kh": 0, "kw": 3, "sh": 1, "sw": 0, "stream": 1, "n_in": pk(9, 9), "n_out": dg(0, 1, 3)} | kw))]
    c["s9_cdg_act"] = (g(act=99, n_in=-1), IMG)
    c["s10_cdg_packed_negative"] = (g(n_in=-1), IMG)
    c["s10b_cdg_packed_n_out_negative"] = (g(n_out=-7), IMG)
    c["s11_cdg_stream"] = (g(), IMG)
    c["s12_cdg_dilation_0"] = (g(stream=0), IMG)
    c["s12b_cdg_dilation_w_0"] = (g(stream=0, n_out=dg(2, 0, 3)), IMG)
    c["s13_cdg_kernel_0"] = (g(stream=0, n_out=dg(2, 1, 3)), IMG)
    c["s13b_cdg_stride_0"] = (g(stream=0, n_out=dg(2, 1, 3), kh=3), IMG)
    c["s14_cdg_groups_cout"] = (g(stream=0, n_out=dg(2, 1, 3), kh=3, sw=1), IMG)
    c["s14b_cdg_groups_0"] = (g(stream=0, n_out=dg(2, 1, 0), kh=3, sw=1), IMG)
    c["s14c_cdg_cin_0"] = (g(stream=0, n_out=dg(2, 1, 1), kh=3, sw=1, cin=0), IMG)
    c["s14d_cdg_groups_cin"] = (g(stream=0, n_out=dg(2, 1, 2), kh=3, sw=1), IMG)
    c["s15_cdg_cin"] = (g(stream=0, n_out=dg(2, 1, 1), kh=3, sw=1), IMG)
    c["s16_cdg_pad_above_extent"] = (g(stream=0, n_out=dg(2, 1, 1), kh=3, sw=1, cin=2), IMG)
    c["s16b_cdg_pad_w_above_extent"] = (g(stream=0, n_out=dg(2, 1, 1), kh=3, sw=1, cin=2, n_in=pk(4, 3)), IMG)
    c["s17_cdg_span_above_map"] = (g(stream=0, n_out=dg(2, 1, 1), kh=5, sw=1, cin=2, n_in=0), IMG)
    c["s17b_cdg_span_w_above_map"] = (g(stream=0, n_out=dg(1, 3, 1), kh=3, kw=4, sw=1, cin=2, n_in=pk(0, 0)), IMG)
    # ---- 18 .. 24: adaptive pools (kh, kw = the output size)
    ap = lambda kind=AMAXP, **kw: R(kind, **({"stream": 1, "act": 1, "cin": 3, "cout": 3, "sh": 1, "kh": 0, "kw": 9} | kw))
    c["s18_apool_stream"] = ([ap()], IMG)
    c["s18b_ameanpool_stream"] = ([ap(AMEANP, stream=2)], IMG)
    for k, (front, kw) in VEC_FRONTS.items():
        c[f"s19_apool_after_{k}"] = (front + [ap(AMEANP if k == "rec" else AMAXP, stream=0)], kw)
    c["s20_apool_act"] = ([ap(stream=0)], IMG)
    c["s21_apool_channels"] = ([ap(AMEANP, stream=0, act=0)], IMG)
    c["s21b_apool_cout_only"] = ([ap(stream=0, act=0, cin=0, cout=2)], IMG)
    c["s22_apool_unused_slots"] = ([ap(stream=0, act=0, cin=2, cout=2)], IMG)
    c["s22b_apool_n_out"] = ([ap(stream=0, act=0, cin=0, cout=0, sh=0, n_out=7)], IMG)
    c["s23_apool_out_0"] = ([ap(stream=0, act=0, cin=0, cout=0, sh=0)], IMG)
    c["s23b_apool_out_w_negative"] = ([ap(AMEANP, stream=0, act=0, cin=0, cout=0, sh=0, kh=9, kw=-1)], IMG)
    c["s24_apool_out_above_map"] = ([ap(stream=0, act=0, cin=0, cout=0, sh=0, kh=1)], IMG)
    c["s24b_apool_out_h_above_map"] = ([cv(2, 4), ap(AMEANP, stream=0, act=0, cin=4, cout=4, sh=0, kh=7, kw=6)], IMG)
    # ---- 25 .. 30: MaxPool / MeanPool
    pl = lambda kind=MAXP, **kw: R(kind, **({"stream": 2, "act": 1, "cin": 3, "cout": 3, "kh": 0, "kw": 2} | kw))
    c["s25_pool_stream"] = ([pl()], IMG)
    c["s25b_meanpool_stream"] = ([pl(MEANP, stream=1)], IMG)
    c["s26_pool_after_dense"] = ([dn(128, 16), pl(stream=0)], IMG)
    c["s26b_meanpool_after_rec"] = ([rec(GRU, 6, 16), pl(MEANP, stream=0)], REC)
    c["s27_pool_act"] = ([pl(stream=0)], IMG)
    c["s28_pool_channels"] = ([pl(MEANP, stream=0, act=0)], IMG)
    c["s28b_pool_cin_only"] = ([pl(stream=0, act=0, cin=2, cout=0)], IMG)
    c["s29_pool_stride_0"] = ([pl(stream=0, act=0, cin=2, cout=2)], IMG)
    c["s29b_pool_stride_w_negative"] = ([pl(stream=0, act=0, cin=0, cout=0, sh=1, sw=-1)], IMG)
    c["s30_pool_window_0"] = ([pl(stream=0, act=0, cin=0, cout=0, sh=1, sw=1)], IMG)
    c["s30b_pool_window_above_map"] = ([cv(2, 4), pl(MEANP, stream=0, act=0, cin=4, cout=4, sh=1, sw=1, kh=6, kw=7)], IMG)
    # ---- 31 .. 42: LayerNorm (eps in cin)
    lnb = lambda **kw: R(LN, **({"n_in": 5, "n_out": 6, "act": 99, "cout": 1, "sw": 2, "cin": f32(-1.0)} | kw))
    c["s31_ln_first"] = ([lnb(stream=1)], VEC)
    c["s32_ln_stream"] = ([first(), lnb(stream=1)], VEC)
    c["s33_ln_after_act"] = ([first(), actl(), lnb()], VEC)
    c["s33b_ln_after_act_on_map"] = ([cv(2, 4), actl(), lnb()], IMG)
    c["s34_ln_after_gn"] = ([cv(2, 4), gn(), lnb()], IMG)
    c["s35_ln_after_conv"] = ([cv(2, 4), lnb()], IMG)
    c["s35b_ln_after_pool"] = ([pool(), lnb()], IMG)
    c["s35c_ln_after_map_join"] = ([cv(2, 4), cv(4, 4, pad=1), skm(1), lnb()], IMG)
    c["s36_ln_after_ln"] = ([first(), ln(16), lnb()], VEC)
    c["s37_ln_n_in_n_out"] = ([first(), lnb()], VEC)
    c["s38_ln_size_1"] = ([first(), lnb(n_in=1, n_out=1)], VEC)
    c["s39_ln_size"] = ([first(), lnb(n_in=12, n_out=12)], VEC)
    c["s40_ln_act"] = ([first(), lnb(n_in=16, n_out=16)], VEC)
    c["s40b_ln_act_11"] = ([first(), lnb(n_in=16, n_out=16, act=11)], VEC)
    c["s41_ln_unused_slots"] = ([first(), lnb(n_in=16, n_out=16, act=1)], VEC)
    c["s41b_ln_kh"] = ([first(), lnb(n_in=16, n_out=16, act=0, cout=0, sw=0, kh=3)], VEC)
    for k, x in (("negative", -1.0), ("inf", float("inf")), ("nan", float("nan")), ("minus_0", -0.0)):
        c["s42_ln_eps_" + k] = ([rec(RNN, 6, 16), lnb(n_in=16, n_out=16, act=1, cout=0, sw=0, cin=f32(x))], REC)
    # ---- 43 .. 53: GroupNorm (G in kh, eps in kw); cv(2, 4) on the (2, 8, 8) observation yields a (4, 6, 6) map, 144 features
    gnb = lambda **kw: R(GN, **({"act": 99, "cin": 3, "cout": 3, "n_in": 5, "n_out": 6, "sh": 1, "sw": 2, "kh": 0, "kw": f32(-2.5)} | kw))
    c["s43_gn_first"] = ([gnb(stream=1)], IMG)
    c["s44_gn_stream"] = ([cv(2, 4), gnb(stream=1)], IMG)
    for k, (front, kw) in VEC_FRONTS.items():
        c[f"s45_gn_after_{k}"] = (front + [gnb()], kw)
    c["s46_gn_act"] = ([cv(2, 4), gnb()], IMG)
    c["s46b_gn_act_11"] = ([cv(2, 4), gnb(act=11)], IMG)
    c["s47_gn_channels"] = ([cv(2, 4), gnb(act=1)], IMG)
    c["s47b_gn_cin_only"] = ([cv(2, 4), gnb(act=1, cin=4, cout=0)], IMG)
    c["s48_gn_n_in_n_out"] = ([cv(2, 4), gnb(act=1, cin=4, cout=4)], IMG)
    c["s49_gn_size"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_out=5)], IMG)
    c["s50_gn_unused_slots"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=144, n_out=144)], IMG)
    c["s50b_gn_sw"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=0, n_out=0, sh=0)], IMG)
    c["s51_gn_G_0"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=0, n_out=0, sh=0, sw=0)], IMG)
    c["s51b_gn_G_divides"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=0, n_out=0, sh=0, sw=0, kh=3)], IMG)
    c["s52_gn_one_element"] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=0, n_out=0, sh=0, sw=0, kh=4)], dict(obs=(2, 3, 3)))
    for k, x in (("negative", -2.5), ("inf", float("inf")), ("nan", float("nan"))):
        c["s53_gn_eps_" + k] = ([cv(2, 4), gnb(act=1, cin=0, cout=0, n_in=0, n_out=0, sh=0, sw=0, kh=2, kw=f32(x))], IMG)
    # ---- 54 .. 64: Dropout (p in cin / cout)
    dob = lambda p=1.0, **kw: R(DO, **({"act": 1, "n_in": 5, "n_out": 6, "kh": 1, "sw": 4, "cin": f64(p)[0], "cout": f64(p)[1]} | kw))
    c["s54_do_first"] = ([dob(stream=1)], VEC)
    c["s55_do_stream"] = ([first(), dob(stream=2)], VEC)
    c["s56_do_after_act"] = ([first(), actl(), dob()], VEC)
    c["s57_do_after_gn"] = ([cv(2, 4), gn(), dob()], IMG)
    c["s58_do_after_conv"] = ([cv(2, 4), dob()], IMG)
    c["s58b_do_after_apool"] = ([apool(1, 1), dob()], IMG)
    c["s59_do_after_do"] = ([first(), do(), dob()], VEC)
    c["s60_do_act"] = ([first(), dob()], VEC)
    c["s61_do_n_in_n_out"] = ([first(), dob(act=0)], VEC)
    c["s62_do_size"] = ([first(), dob(act=0, n_out=5)], VEC)
    c["s63_do_unused_slots"] = ([first(), dob(act=0, n_in=16, n_out=16)], VEC)
    c["s63b_do_sh"] = ([first(), ln(16), dob(act=0, n_in=0, n_out=0, kh=0, sw=0, sh=7)], VEC)
    for k, x in (("one", 1.0), ("negative", -0.5), ("nan", float("nan")), ("two", 2.0)):
        c["s64_do_p_" + k] = ([first(), dob(x, act=0, n_in=0, n_out=0, kh=0, sw=0)], VEC)
    # ---- 65 .. 81: the join of a convolutional skip block (m in cin)
    jm = lambda **kw: R(SKM, **({"act": 1, "cin": 0, "cout": 1, "kh": 2, "kw": 3, "sh": 4, "sw": 5, "n_in": 5, "n_out": 6} | kw))
    blk = lambda: [cv(2, 4), cv(4, 4, pad=1)]
    c["s65_skm_stream"] = (blk() + [jm(stream=1)], IMG)
    c["s66_skm_act"] = (blk() + [jm()], IMG)
    c["s67_skm_m_0"] = (blk() + [jm(act=0)], IMG)
    c["s67b_skm_m_negative"] = (blk() + [jm(act=0, cin=-2)], IMG)
    c["s68_skm_unused_slots"] = (blk() + [jm(act=0, cin=9)], IMG)
    c["s69_skm_m_above_i"] = (blk() + [jm(act=0, cin=9, cout=0, kh=0, kw=0, sh=0, sw=0)], IMG)
    j1 = lambda m=1: jm(act=0, cin=m, cout=0, kh=0, kw=0, sh=0, sw=0)      # the join's own slots in order but for (n_in, n_out) = (5, 6)
    c["s70_skm_inner_stream"] = ([cv(2, 4), dn(144, 16, stream=1), j1()], IMG)
    c["s70b_skm_inner_order"] = ([cv(2, 4), cv(4, 4, k=1), dn(144, 16, stream=1), j1(2)], IMG)      # the FIRST inner layer answers (a pad-0 Conv), not the first rule
    c["s71_skm_nested"] = (blk() + [skm(1), cv(4, 4, pad=1), j1(3)], IMG)
    c["s71b_skm_across_vector_join"] = ([first(), dn(16, 16), sk(1), j1(1)], VEC)
    c["s72_skm_inner_act"] = (blk() + [actl(), j1(2)], IMG)
    c["s73_skm_inner_pool"] = (blk() + [pool(k=1, s=1), j1(2)], IMG)
    c["s73b_skm_inner_apool"] = (blk() + [apool(6, 6), j1(2)], IMG)
    c["s74_skm_inner_cdg"] = ([cv(2, 4), cdg(4, 4, pad=(2, 2), dil=(2, 2)), j1()], IMG)
    c["s75_skm_inner_conv_pad_0"] = ([cv(2, 4), cv(4, 4, k=1), j1()], IMG)
    c["s76_skm_inner_dense"] = ([cv(2, 4), dn(144, 144), j1()], IMG)
    c["s76b_skm_inner_gn"] = ([cv(2, 4), gn(), j1()], IMG)
    c["s76c_skm_inner_ln"] = ([cv(2, 4), dn(144, 16), ln(16), j1()], IMG)
    c["s76d_skm_inner_do"] = ([cv(2, 4), dn(144, 16), do(), j1()], IMG)
    c["s76e_skm_inner_rec"] = ([cv(2, 4), rec(LSTM, 144, 8), j1()], IMG | dict(recurrence=1, trace_length=3))
    c["s77_skm_reads_observation"] = ([cv(2, 2, pad=1), j1()], IMG)
    for k, (front, kw) in VEC_FRONTS.items():
        c[f"s78_skm_on_{k}"] = (front + [cv(16, 16, pad=1), j1()], kw)
    c["s79_skm_shape"] = ([cv(2, 4), cv(4, 8, pad=1), j1()], IMG)
    c["s79b_skm_shape_stride"] = ([cv(2, 4), cv(4, 4, s=2, pad=1), j1()], IMG)
    c["s80_skm_n_in_n_out"] = (blk() + [j1()], IMG)
    c["s81_skm_size"] = (blk() + [skm(1, 5)], IMG)
    # ---- 82 .. 99: the join of a skip block on a feature vector
    jv = lambda **kw: R(SK, **({"act": 1, "cin": 0, "cout": 1, "kh": 2, "kw": 3, "sh": 4, "sw": 5, "n_in": 5, "n_out": 6} | kw))
    vb = lambda: [first(), dn(16, 16)]
    v1 = lambda m=1: jv(act=0, cin=m, cout=0, kh=0, kw=0, sh=0, sw=0)
    c["s82_sk_stream"] = (vb() + [jv(stream=2)], VEC)
    c["s83_sk_act"] = (vb() + [jv()], VEC)
    c["s84_sk_m_0"] = (vb() + [jv(act=0)], VEC)
    c["s85_sk_unused_slots"] = (vb() + [jv(act=0, cin=9)], VEC)
    c["s86_sk_m_above_i"] = (vb() + [v1(9)], VEC)
    c["s87_sk_inner_stream"] = ([first(), dn(16, 16, stream=1), v1()], VEC)
    c["s87b_sk_inner_order"] = ([first(), rec(RNN, 16, 16), dn(16, 16, stream=2), v1(2)], REC)      # the FIRST inner layer answers (a recurrent layer)
    c["s88_sk_nested"] = (vb() + [sk(1), dn(16, 16), v1(3)], VEC)
    c["s88b_sk_across_map_join"] = ([cv(2, 4), cv(4, 4, pad=1), skm(1), v1()], IMG)
    c["s89_sk_inner_rec"] = ([first(), rec(GRU, 16, 16), v1()], REC)
    c["s90_sk_inner_act"] = (vb() + [actl(), v1(2)], VEC)
    c["s91_sk_inner_gn"] = ([cv(2, 4), gn(), v1()], IMG)
    c["s92_sk_inner_cdg"] = ([cv(2, 4), cdg(4, 4), v1()], IMG)
    c["s93_sk_inner_conv"] = ([cv(2, 4), cv(4, 4, pad=1), v1()], IMG)
    c["s93b_sk_inner_pool"] = ([cv(2, 4), pool(), v1()], IMG)
    c["s94_sk_reads_observation"] = ([dn(6, 6), v1()], VEC)
    c["s95_sk_on_gn"] = ([cv(2, 4), gn(), dn(144, 144), v1()], IMG)
    c["s96_sk_on_conv"] = ([cv(2, 4), dn(144, 144), v1()], IMG)
    c["s96b_sk_on_act_on_map"] = ([cv(2, 4), actl(), dn(144, 144), v1()], IMG)
    c["s97_sk_n_to_m"] = ([first(), dn(16, 12), v1()], VEC)
    c["s98_sk_n_in_n_out"] = (vb() + [v1()], VEC)
    c["s99_sk_size"] = (vb() + [sk(1, 5)], VEC)
    # ---- 100 .. 105: the standalone activation layer
    ab = lambda **kw: R(ACT, **({"act": 99, "n_in": 5, "n_out": 6, "cin": 1, "cout": 2, "kh": 3, "kw": 4, "sh": 5, "sw": 6} | kw))
    c["s100_act_first"] = ([ab(stream=1)], VEC)
    c["s101_act_stream"] = ([first(), ab(stream=1)], VEC)
    c["s102_act_code"] = ([first(), ab()], VEC)
    c["s102b_act_code_15"] = ([first(), ab(act=15)], VEC)
    c["s102c_act_code_negative"] = ([cv(2, 4), ab(act=-1)], IMG)
    c["s103_act_n_in_n_out"] = ([first(), ab(act=14)], VEC)
    c["s104_act_size"] = ([cv(2, 4), ab(act=14, n_out=5)], IMG)
    c["s105_act_unused_slots"] = ([first(), ab(act=14, n_in=16, n_out=16)], VEC)
    c["s105b_act_sw"] = ([cv(2, 4), ab(act=0, n_in=144, n_out=144, cin=0, cout=0, kh=0, kw=0, sh=0)], IMG)
    # ---- 106, 107: Dense
    c["s106_dense_act"] = ([dn(7, 4, act=99)], VEC)
    c["s106b_dense_act_11"] = ([first(), dn(7, 4, act=11)], VEC)
    c["s107_dense_n_in"] = ([dn(7, 4, act=10)], VEC)
    c["s107b_dense_n_in_after_map"] = ([cv(2, 4), dn(143, 4)], IMG)
    # ---- 108 .. 111: recurrent layers
    for k, kind in (("lstm", LSTM), ("gru", GRU), ("rnn", RNN)):
        c[f"s108_{k}_recurrence_off"] = ([rec(kind, 7, 8, stream=1, act=99)], VEC)
        c[f"s109_{k}_stream"] = ([rec(kind, 7, 8, stream=1, act=99)], REC)
        c[f"s110_{k}_n_in"] = ([rec(kind, 7, 8, act=99)], REC)
    c["s111_rnn_act"] = ([rec(RNN, 6, 8, act=4), dn(8, 4)], REC)
    c["s111b_rnn_act_negative"] = ([first(), rec(RNN, 16, 8, act=-1), dn(8, 4)], REC)
    # ---- 112: no such kind
    c["s112_unknown_kind"] = ([first(), R(99, n_in=16, n_out=4)], VEC)
    c["s112b_unknown_kind_negative"] = ([R(-1, n_in=6, n_out=4)], VEC)
    # ---- 113 .. 116: behind the loop
    c["s113_dueling_no_streams"] = ([first(), dn(16, 4)], VEC | dict(dueling=1))
    c["s113b_dueling_value_width"] = ([first(), dn(16, 2, stream=1), dn(16, 4, stream=2)], VEC | dict(dueling=1))
    c["s113c_dueling_advantage_width"] = ([first(), dn(16, 1, stream=1), dn(16, 5, stream=2)], VEC | dict(dueling=1))
    c["s113d_dueling_no_advantage"] = ([first(), dn(16, 1, stream=1)], VEC | dict(dueling=1))
    c["s114_output_size"] = ([first(), dn(16, 5)], VEC)
    c["s114b_output_size_before_kind"] = ([first(), dn(16, 5), ln(5)], VEC)
    c["s114c_streams_without_dueling"] = ([dn(6, 3), dn(3, 1, stream=1), dn(3, 4, stream=2)], VEC)
    c["s115_output_gn"] = ([cv(2, 4, k=8), gn(1)], IMG)
    c["s115b_output_act"] = ([first(), dn(16, 4), actl()], VEC)
    c["s115c_output_apool"] = ([cv(2, 4), apool(1, 1, AMEANP)], IMG)
    c["s115d_output_map_join"] = ([cv(2, 4, k=8), cv(4, 4, pad=1), skm(1)], IMG)
    c["s115e_output_before_n_actions"] = ([first(), dn(16, 65), ln(65)], VEC | dict(n_actions=65))
    c["s116_n_actions"] = ([first(), dn(16, 65)], VEC | dict(n_actions=65))
    c["s116b_n_actions_dueling"] = ([first(), dn(16, 1, stream=1), dn(16, 65, stream=2)], VEC | dict(n_actions=65, dueling=1))
    return c


def _accepted():
    """name -> (front, tail, hparams): every prefix of `front` is probed; front + tail is a whole network"""
    c = {}
    O97 = dict(obs=(2, 9, 7))
    cvx = lambda ci, co, kh, kw, sh=1, sw=1, ph=0, pw=0, **kw_: R(CV, cin=ci, cout=co, kh=kh, kw=kw, sh=sh, sw=sw, n_in=ph, n_out=pw, **kw_)
    gx = lambda ci, co, kh, kw, sh=1, sw=1, pad=(0, 0), dil=(1, 1), g=1, **kw_: R(CDG, cin=ci, cout=co, kh=kh, kw=kw, sh=sh, sw=sw, n_in=pk(*pad), n_out=dg(*dil, g), **kw_)
    # Conv: non-square map, kernel and stride; trailing rows / columns no window covers
    c["conv_nonsquare"] = ([cvx(2, 5, 3, 2, 2, 1, act=1)], [dn(120, 4)], O97)                            # (5, 4, 6)
    c["conv_trailing"] = ([cvx(2, 3, 4, 3, 3, 3, act=2)], [dn(12, 4)], O97)                              # (3, 2, 2): rows 7, 8 and column 6 are dropped
    c["conv_whole_map"] = ([cvx(2, 4, 9, 7, 5, 5)], [], O97)                                             # (4, 1, 1) = n_actions: a Conv may be the output layer
    c["conv_conv"] = ([cvx(2, 4, 3, 3, act=1), cvx(4, 6, 2, 3, 2, 1, act=10)], [dn(54, 4)], O97)         # (4, 7, 5) -> (6, 3, 3)
    # padded Conv: the issue's example; pad at its maximum kernel - 1; one axis padded; stride with pad
    c["cpad_3x3_s2"] = ([cvx(2, 5, 3, 3, 2, 2, 1, 1, act=1)], [dn(100, 4)], O97)                         # (5, 5, 4)
    c["cpad_max"] = ([cvx(2, 3, 3, 2, 1, 1, 2, 1, act=1)], [dn(264, 4)], O97)                            # (3, 11, 8)
    c["cpad_one_axis"] = ([cvx(2, 3, 3, 3, 2, 3, 0, 2, act=3)], [dn(36, 4)], O97)                        # (3, 4, 3)
    c["cpad_h_only"] = ([cvx(2, 3, 2, 1, 1, 1, 1, 0)], [dn(210, 4)], O97)                                # (3, 10, 7)
    c["cpad_after_pool"] = ([R(MEANP, kh=2, kw=2, sh=2, sw=2), cvx(2, 4, 3, 3, 1, 1, 1, 1, act=1)], [dn(48, 4)], O97)      # (2, 4, 3) -> (4, 4, 3)
    # dilated / grouped Conv: dilation with pad, groups, depthwise, stride, pad at the dilated extent - 1
    c["cdg_dilation_pad"] = ([gx(2, 4, 3, 3, pad=(2, 1), dil=(2, 1), act=1)], [dn(252, 4)], O97)         # (4, 9, 7)
    c["cdg_groups"] = ([gx(2, 4, 3, 2, g=2, act=1)], [dn(168, 4)], O97)                                  # (4, 7, 6), K = 1 * 3 * 2
    c["cdg_depthwise_stride"] = ([gx(2, 2, 3, 3, 2, 3, dil=(1, 2), g=2)], [dn(8, 4)], O97)               # spans (3, 5): (2, 4, 1)
    c["cdg_pad_max"] = ([gx(2, 2, 2, 3, pad=(3, 4), dil=(3, 2), act=5)], [dn(264, 4)], O97)              # extents (4, 5), pad = extent - 1: (2, 12, 11)
    c["cdg_plain"] = ([gx(2, 4, 3, 3, 2, 2)], [dn(48, 4)], O97)                                          # dilation 1, groups 1, pad 0: a Conv's geometry, (4, 4, 3)
    c["cdg_stack"] = ([cvx(2, 4, 3, 3, act=1), gx(4, 8, 3, 3, pad=(1, 1), g=4, act=1), gx(8, 8, 2, 2, dil=(2, 2), g=8)], [dn(120, 4)], O97)      # (4, 7, 5) -> (8, 7, 5) -> (8, 5, 3)
    # pools
    c["pool_nonsquare"] = ([cvx(2, 4, 2, 2, act=1), R(MAXP, kh=3, kw=2, sh=2, sw=3)], [dn(24, 4)], O97)  # (4, 8, 6) -> (4, 3, 2)
    c["pool_first_trailing"] = ([R(MEANP, cin=2, cout=2, kh=4, kw=3, sh=4, sw=2)], [dn(12, 4)], O97)     # (2, 2, 3): row 8 is dropped
    c["pool_overlap"] = ([R(MAXP, kh=3, kw=3, sh=1, sw=2)], [dn(42, 4)], O97)                            # (2, 7, 3)
    # adaptive pools: Flux's rule (stride = in / out, k = in - (out - 1) * stride), NOT torch's; out == in; global
    c["apool_indivisible"] = ([apool(4, 3)], [dn(24, 4)], O97)                                           # 9 -> 4: stride 2, k 3; 7 -> 3: stride 2, k 3
    c["apool_mean_channels_given"] = ([cvx(2, 4, 2, 2, act=1), apool(3, 4, AMEANP, cin=4, cout=4)], [dn(48, 4)], O97)      # (4, 8, 6) -> (4, 3, 4)
    c["apool_identity"] = ([apool(9, 7, AMEANP)], [dn(126, 4)], O97)
    c["apool_global"] = ([cvx(2, 8, 3, 3, act=1), apool(1, 1)], [dn(8, 4)], O97)
    c["apool_global_mean_first"] = ([apool(1, 1, AMEANP)], [dn(2, 4)], O97)
    c["apool_one_axis"] = ([apool(1, 5)], [dn(10, 4)], O97)
    # GroupNorm, Activation and both joins keep the map
    c["gn_keeps_map"] = ([cvx(2, 4, 3, 2, 2, 1), gn(2, act=1)], [dn(96, 4)], O97)                        # (4, 4, 6)
    c["gn_slots_given"] = ([cvx(2, 6, 3, 3), R(GN, cin=6, cout=6, n_in=210, n_out=210, kh=3, kw=f32(1e-3), act=10), gn(6), R(MAXP, kh=2, kw=2, sh=2, sw=2)], [dn(36, 4)], O97)      # (6, 7, 5) -> (6, 3, 2)
    c["gn_after_pool"] = ([R(MAXP, kh=2, kw=2, sh=2, sw=2), gn(1)], [dn(24, 4)], O97)
    c["act_keeps_map"] = ([cvx(2, 4, 3, 2, 2, 1), actl(12), cvx(4, 2, 2, 2), actl(14, n_in=30, n_out=30), gn(2)], [dn(30, 4)], O97)      # (4, 4, 6) -> (2, 3, 5)
    c["skm_keeps_map"] = ([cvx(2, 4, 3, 3, act=1), cvx(4, 4, 3, 3, 1, 1, 1, 1), skm(1)], [dn(140, 4)], O97)      # (4, 7, 5)
    c["skm_two_inner_size_given"] = ([R(MAXP, kh=2, kw=2, sh=2, sw=2), cvx(2, 2, 3, 1, 1, 1, 1, 0, act=1), cvx(2, 2, 1, 3, 1, 1, 0, 1), skm(2, 24), R(MEANP, kh=2, kw=1, sh=2, sw=1)], [dn(12, 4)], O97)
    c["skm_on_skm"] = ([cvx(2, 4, 3, 3, act=1), cvx(4, 4, 3, 3, 1, 1, 1, 1), skm(1), cvx(4, 4, 3, 3, 1, 1, 1, 1, act=1), skm(1), gn(4)], [dn(140, 4)], O97)
    c["skm_then_global_pool"] = ([cvx(2, 4, 3, 3, act=1), cvx(4, 4, 3, 3, 1, 1, 1, 1), skm(1), apool(1, 1, AMEANP)], [dn(4, 4)], O97)
    # on a feature vector: LayerNorm, Dropout, Activation, the join; the (n, 1, 1) reading (Conv 1x1 after LayerNorm, pool 1x1 behind it)
    c["ln_do_act_on_vector"] = ([first(), ln(16, act=7), do(), dn(16, 12, act=1), actl(13), dn(12, 12), R(DO, n_in=12, n_out=12, cin=f64(0.25)[0], cout=f64(0.25)[1]),
                                 R(LN, n_in=12, n_out=12, cin=f32(1e-3))], [dn(12, 4)], VEC)
    c["sk_on_vector"] = ([first(), ln(16), dn(16, 16, act=1), do(), sk(3), dn(16, 8), dn(8, 8, act=2), sk(1, 8), actl(0)], [dn(8, 4)], VEC)
    c["vector_as_map"] = ([first(), ln(16), cvx(16, 8, 1, 1, act=1), R(MAXP, kh=1, kw=1, sh=1, sw=1), cvx(8, 6, 1, 1, 1, 1, 0, 0), apool(1, 1), gx(6, 6, 1, 1, g=3)], [dn(6, 4)], VEC)
    c["dense_after_map_act"] = ([cvx(2, 4, 3, 3), actl(11), dn(140, 16, act=9)], [dn(16, 4)], O97)
    # recurrent layers (an LSTM / GRU ignores act: the cell has none of its own to choose)
    c["lstm"] = ([rec(LSTM, 6, 8, act=99), ln(8)], [dn(8, 4)], REC)
    c["gru"] = ([first(), rec(GRU, 16, 12, act=-3), do()], [dn(12, 4)], REC)
    c["rnn_act"] = ([rec(RNN, 6, 8, act=3), rec(RNN, 8, 10, act=0), actl(1)], [dn(10, 4)], REC)
    c["rec_stack_after_conv"] = ([cvx(2, 3, 4, 3, 3, 3), rec(LSTM, 12, 8), rec(GRU, 8, 8), rec(RNN, 8, 5, act=2)], [dn(5, 4)], O97 | dict(recurrence=1, trace_length=2))
    c["lstm_output"] = ([rec(LSTM, 6, 4)], [], REC)
    # a dueling split: base chain, then a value and an advantage stream
    c["dueling_dense"] = ([first(), dn(16, 8, act=1, stream=1), dn(16, 12, act=1, stream=2), dn(8, 1, stream=1), dn(12, 4, stream=2)], [], VEC | dict(dueling=1))
    c["dueling_after_conv"] = ([cvx(2, 4, 3, 3, 2, 2, act=1), dn(48, 32, act=1), dn(32, 8, act=1, stream=2), dn(32, 6, act=1, stream=1), dn(8, 4, stream=2), dn(6, 1, stream=1)], [], O97 | dict(dueling=1))
    c["dueling_split_at_map"] = ([cvx(2, 4, 3, 3, 2, 2, act=1), cvx(4, 2, 2, 2, stream=1, act=1), dn(48, 4, stream=2), dn(12, 1, stream=1)], [], O97 | dict(dueling=1))
    # wide layers, so that the plan rules that read K, N and npos have something to cut
    c["wide_dense"] = ([dn(6, 2048, act=1), dn(2048, 600, act=1), actl(11), dn(600, 256, act=1)], [dn(256, 4)], VEC)
    c["wide_conv"] = ([cvx(2, 32, 3, 3, 1, 1, 1, 1, act=1), gx(32, 64, 3, 3, 2, 2, pad=(1, 1), g=2, act=1), cvx(64, 64, 3, 2, act=1), gn(8), R(MAXP, kh=2, kw=2, sh=1, sw=1)], [dn(1280, 512, act=1), dn(512, 4)], dict(obs=(2, 16, 12)))
    return c


REFUSED = _refusals()
ACCEPTED = _accepted()
# the refusal sites of build_layers on the recorded commit, in the function's order; every one is reached by the case(s) named s<site>..., none is unreachable
SITES = 116
PROBES = {"conv": lambda s: R(CV, stream=s, cin=-1, cout=1, kh=1, kw=1, sh=1, sw=1), "pool": lambda s: R(MAXP, stream=s, kh=9999, kw=9999, sh=1, sw=1), "dense": lambda s: dn(-1, 1, stream=s)}


def site_of(name):
    """s76b_skm_inner_gn -> 76"""
    return int(name[1:].split("_")[0].rstrip("abcdefgh"))


def _hp(kw, B):
    kw = dict(kw); obs = kw.pop("obs")
    return pkg.default_hparams(**({"batch_size": B, "n_actions": 4, "obs_c": obs[0], "obs_h": obs[1], "obs_w": obs[2], "buffer_size": 256, "dueling": 0} | kw))


def _ask(layers, hp):
    try:
        return {"plan": [list(p) for p in pkg.default_plan(layers, hp)]}
    except pkg.DQNError as e:
        return {"error": str(e)}


def observe(name):
    if name in REFUSED:
        layers, kw = REFUSED[name]
        return _ask(layers, _hp(kw, 8))      # a refusal needs one batch size: build_layers does not read it
    front, tail, kw = ACCEPTED[name]
    out = {"B8": _ask(front + tail, _hp(kw, 8)), "B128": _ask(front + tail, _hp(kw, 128)), "probes": []}
    for n in range(1, len(front) + 1):
        streams = sorted({d.stream for d in front[:n]})
        row = {f"{p}@{s}": _ask(front[:n] + [make(s)], _hp(kw, 8)).get("error") for p, make in PROBES.items() for s in streams if s == 0 or p == "dense"}
        out["probes"].append(row)
    return out


if __name__ == "__main__":      # python tests/build_layers_cases.py > tests/golden/build_layers_cpu.json (docs/history/build_layers.md)
    import json
    import sys
    json.dump({n: observe(n) for n in list(REFUSED) + list(ACCEPTED)}, sys.stdout, indent=0, sort_keys=True)
    sys.stdout.write("\n")
