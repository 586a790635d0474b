# Every translation unit of libhz and every header they include, relative to
# this folder: the one list behind libhz.so (../Makefile) and the whole-library
# diagnostic variants (tools/Makefile).  A new unit or header is named here only.
HZ_UNITS := hz_env hz_mcts hz_mcts_report hz_mcts_carry hz_turn hz_draws hz_net hz_net_wide hz_train
HZ_HDRS := hz_device.hpp hz_initgen.hpp hz_encode.hpp hz_host.hpp hz_chance.hpp hz_rollout.hpp hz_play2.hpp \
	hz_sym.hpp hz_mcts.hpp ../../include/hz_abi.h
